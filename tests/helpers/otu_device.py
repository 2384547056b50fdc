"""Crafted batches, the host writer's answer and the test bodies of smr_otu_part / smr_fastx_denovo (test_gpu_otu_device.py runs them on the
GPU, test_emu_otu_device.py on the kernel emulator).  TEST INFRASTRUCTURE ONLY.

The yardstick is always the host writer: the same reads and records go through smr_report_add / smr_report_add_pair into a temporary
directory, and what it wrote is compared with what the device's streams give through smr_report_add_otu / smr_report_add_denovo."""
import ctypes as C
import os
import struct

import numpy as np

import sortmerna_amd as smr
from sortmerna_amd import report

from . import fxsplit, golden, otu, rows

ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -4, -5
KEYS = [(0, 0), (1, 0)]                     # the crafted records spread their alignments over these two keys; both are registered with the same index part
N_REFS = 1100                               # more than 1025 (every pair its own group) and than 256 (a second digit pass of the sort)
SORT_NS = [0, 1, 63, 64, 65, 4097, 100003]
PAIR_COUNTS = [0, 1, 63, 64, 65, 1025]
ALL_KINDS = {"two to one reference", "two to two references", "passing and failing", "strand 0, forward letters equal", "strand 0, a true reverse complement", "N against N",
             "more than 64 operations"}
SHAPES = ["one", "own", "mixed"]
_db = {}


# ------------------------------------------------------------------------------------------------ the crafted database
def crafted_db():
    """-> (Index part, [reference letters]): N_REFS references; 0 is long (a CIGAR of more than 64 operations, a 1000-letter read), 1 begins
    with the nine letters of reference 0 at 100 (the second rounding), 3 holds runs of N; built once per process"""
    if "ix" not in _db:
        import atexit, shutil, tempfile
        d = tempfile.mkdtemp(prefix="smr_otu_dev_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        rng = np.random.Generator(np.random.PCG64(77))
        refs = []
        for r in range(N_REFS):
            L = 2400 if r == 0 else int(rng.integers(110, 180))
            refs.append("".join("ACGT"[int(c)] for c in rng.integers(0, 4, L)))
        refs[1] = refs[0][100:109] + refs[1][9:]
        s = list(refs[3])
        for k in (5, 6, 40, 41, 42, 90):
            s[k] = "N"
        refs[3] = "".join(s)
        path = os.path.join(d, "db.fasta")
        with open(path, "w") as f:
            for r, s in enumerate(refs):
                f.write(">ref%04d some description\n%s\n" % (r, s))
        _db["ix"] = smr.Index.build(path, 18, 3072.0, 10000, 0)[0]
        _db["refs"] = refs
    return _db["ix"], _db["refs"]


def m_aln(ref_num, ref_begin, n, read_begin, readlen, key=(0, 0), strand=1, cigar=None, ref_span=None):
    return dict(cigar=cigar if cigar is not None else [(n << 4) | 0], ref_num=ref_num, ref_begin1=ref_begin, ref_end1=ref_begin + (ref_span or n) - 1,
                read_begin1=read_begin, read_end1=read_begin + n - 1, readlen=readlen, score1=2 * n, part=key[1], index_num=key[0], strand=strand)


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def header_of(i, kind):
    forms = ["r%d", "r%d some words", "r%d\tTAB before a space", ">r%d", "@r%d x", "r%d ", "r%d  two", "%d"]
    if kind == "short":
        return "abcdefghij"[i % 10]                                 # an id of one byte
    if kind == "long":
        return "L%d_" % i + "x" * (4100 + i % 7) + " behind the id"  # longer than the LDS window
    return forms[i % len(forms)] % i


class Batch:
    """reads (header, letters) with their crafted alignments -> FASTX text and records"""
    def __init__(self, fastq, slots=4):
        self.fastq, self.slots, self.reads, self.kinds = fastq, slots, [], {}

    def add(self, header, seq, alns):
        assert len(alns) <= self.slots
        self.reads.append((header, seq, alns))

    def mark(self, kind):
        self.kinds.setdefault(kind, []).append(len(self.reads) - 1)     # the read added last is of this kind

    def text(self):
        out = []
        for i, (h, s, _) in enumerate(self.reads):
            out.append(("@%s\n%s\n+\n%s\n" % (h, s, "".join(chr(33 + (j + i) % 40) for j in range(len(s))))) if self.fastq else (">%s\n%s\n" % (h, s)))
        return "".join(out).encode()

    def records(self):
        return [rows.record(a, self.slots) for _, _, a in self.reads]


def craft(n_pairs, shape, fastq, seed=1):
    """a batch whose map (thresholds 0.9 / 0.4) holds exactly n_pairs members over the two keys.  one: all in the group of one reference;
    own: every member a group of its own, the references descending; mixed: reads with two passing alignments (to one and to two references),
    with a passing and a failing one, with none, on the reverse strand (forward letters equal: passes; a true reverse complement: does not),
    with N against N, alignments of the second key, ids of one byte and of more than 4096"""
    _, refs = crafted_db()
    rng = np.random.Generator(np.random.PCG64(seed))
    B = Batch(fastq)
    made = 0

    def piece(r, L):
        b = int(rng.integers(0, len(refs[r]) - L + 1))
        return b, refs[r][b:b + L]

    i = 0
    while made < n_pairs or i < 3:
        kind = "short" if i % 17 == 3 else "long" if i % 41 == 7 else ""
        h = header_of(i, kind)
        if shape == "one" or shape == "own":
            if made >= n_pairs:
                break
            r = 7 if shape == "one" else (n_pairs - 1 - made) + 4
            b, s = piece(r, 100)
            B.add(h, s, [m_aln(r, b, 100, 0, 100)])
            made += 1
        else:
            k = i % 9 if i < 18 else int(rng.integers(0, 9))            # every kind twice in the first 18 reads, whatever the seed; then at random
            coin = i < 9 if i < 18 else bool(rng.integers(0, 2))
            left = n_pairs - made
            if k == 0 and left >= 2:                               # two halves on two references (or twice the same one)
                r1 = int(rng.integers(4, N_REFS)); r2 = r1 if coin else (r1 - 4 + 1 + int(rng.integers(0, N_REFS - 5))) % (N_REFS - 4) + 4
                (b1, s1), (b2, s2) = piece(r1, 50), piece(r2, 50)
                B.add(h, s1 + s2, [m_aln(r1, b1, 50, 0, 100, key=KEYS[int(rng.integers(0, 2))]), m_aln(r2, b2, 50, 50, 100)])
                made += 2; B.mark("two to one reference" if coin else "two to two references")
            elif k == 1 and left >= 1:                             # a passing and a failing alignment: the read's counter is above 0, the second is classified again
                r1, r2 = int(rng.integers(4, N_REFS)), int(rng.integers(4, N_REFS))
                b1, s1 = piece(r1, 100)
                B.add(h, s1, [m_aln(r2, 3, 100, 0, 100), m_aln(r1, b1, 100, 0, 100)])
                made += 1; B.mark("passing and failing")
            elif k == 2:                                           # no passing alignment at all: c_yid_ycov stays 0
                r1 = int(rng.integers(4, N_REFS))
                B.add(h, "".join("ACGT"[int(c)] for c in rng.integers(0, 4, 100)), [m_aln(r1, 2, 100, 0, 100)])
            elif k == 3:                                           # no alignment
                B.add(h, "ACGTTGCA" * 10, [])
            elif k == 4 and left >= 1:                             # strand 0 with the FORWARD letters equal: passes (the reproduced quirk); a true reverse alignment does not
                r1 = int(rng.integers(4, N_REFS))
                b1, s1 = piece(r1, 100)
                if coin:
                    B.add(h, s1, [m_aln(r1, b1, 100, 0, 100, strand=0)]); made += 1; B.mark("strand 0, forward letters equal")
                else:
                    B.add(h, revcomp(s1), [m_aln(r1, b1, 100, 0, 100, strand=0)]); B.mark("strand 0, a true reverse complement")
            elif k == 5 and left >= 1:                             # an ambiguous read letter against a reference N (equal), and one against a base (not)
                s = list(refs[3][:100]); s[20] = "N"
                B.add(h, "".join(s), [m_aln(3, 0, 100, 0, 100, key=KEYS[1])]); made += 1; B.mark("N against N")
            elif k == 6 and left >= 1:                             # a CIGAR of more than 64 operations: 20 M then an insertion / a deletion, 36 times
                cig, rd, q = [], [], 200
                for j in range(36):
                    cig.append((20 << 4) | 0); rd.append(refs[0][q:q + 20]); q += 20
                    if j % 2 == 0:
                        cig.append((1 << 4) | 1); rd.append("A")
                    else:
                        cig.append((1 << 4) | 2); q += 1
                s = "".join(rd)
                assert len(cig) > 64
                B.add(h, s, [m_aln(0, 200, len(s), 0, len(s), cigar=cig, ref_span=q - 200)]); made += 1; B.mark("more than 64 operations")
            elif left >= 1:
                r1 = int(rng.integers(4, N_REFS))
                L = int(rng.integers(60, 110))
                b1, s1 = piece(r1, L)
                B.add(h, s1, [m_aln(r1, b1, L, 0, L, key=KEYS[int(rng.integers(0, 4) == 0)])]); made += 1
            elif made >= n_pairs and i >= 3:
                break
        i += 1
    if not B.reads:
        B.add("lonely", "ACGTTGCA" * 10, [m_aln(9, 2, 80, 0, 80)])
    return B


# ------------------------------------------------------------------------------------------------ host and device reports
def open_report(tmpdir, fastq, reg, min_id, min_cov, **kw):
    os.makedirs(str(tmpdir), exist_ok=True)
    rep = report.Report(str(tmpdir), is_fastq=fastq, fastx=False, other=False, otu_map=True, denovo=True, min_id=min_id, min_cov=min_cov, **kw)
    for (k, part), ix in reg.items():
        rep.set_part(k, part, ix)
    return rep


def map_file(tmpdir):
    p = os.path.join(str(tmpdir), "otu_map.txt")
    return open(p, "rb").read() if os.path.isfile(p) else None


def denovo_files(tmpdir, fastq, n_out_sfx=("",)):
    out = []
    for sfx in n_out_sfx:
        p = os.path.join(str(tmpdir), "aligned_denovo" + sfx + (".fq" if fastq else ".fa"))
        out.append(open(p, "rb").read() if os.path.isfile(p) else None)
    return out


def host_report(tmpdir, reads, recs, fastq, reg, min_id, min_cov):
    """the per-read host loop -> (otu_map.txt or None, total_otu, aligned_denovo)"""
    rep = open_report(tmpdir, fastq, reg, min_id, min_cov)
    for i, rec in enumerate(recs):
        hdr, seq, qual = reads.record_text(i)
        rep.add(hdr, seq, qual, rec)
    rep.close()
    return map_file(tmpdir), rep.total_otu, denovo_files(tmpdir, fastq)[0]


def device_report(tmpdir, e, fastq, reg, params_of, min_id, min_cov, slot_of=None, results=None):
    """smr_otu_part per (index, part) + smr_report_add_otu, smr_fastx_denovo + smr_report_add_denovo, in a report that skips both -> the same triple"""
    rep = open_report(tmpdir, fastq, reg, min_id, min_cov)
    rep.skip_otu()
    rep.skip_denovo()
    for key, ix in reg.items():
        p = params_of(key)
        p.index_num, p.part = key
        data, groups, any_ = e.otu_part(slot_of(key) if slot_of else 0, p, ix, min_id, min_cov)
        check_groups(data, groups)
        if results is not None:
            results[key] = (data, groups, any_)
        rep.add_otu(key[0], key[1], data, groups, any_)
    rep.add_denovo(e.fastx_denovo())
    rep.close()
    return map_file(tmpdir), rep.total_otu, denovo_files(tmpdir, fastq)[0]


def check_groups(data, groups):
    """ascending references, offsets that rise, as many ids as members"""
    for g in range(len(groups)):
        assert g == 0 or int(groups[g]["ref_num"]) > int(groups[g - 1]["ref_num"]), "groups are not ascending in ref_num"
        b = int(groups[g]["off"]); e_ = int(groups[g + 1]["off"]) if g + 1 < len(groups) else len(data)
        assert b <= e_ <= len(data) and int(groups[g]["n_reads"]) >= 1
        assert not data[b:e_].endswith(b"\t") or int(groups[g]["n_reads"]) > data[b:e_].count(b"\t")
    assert len(groups) == 0 or int(groups[0]["off"]) == 0


def run_pass(e, reg, params_of, min_id, min_cov, slot_of=None):
    for key in reg:
        p = params_of(key)
        p.index_num, p.part = key
        e.idcov_part(slot_of(key) if slot_of else 0, p, min_id, min_cov)


def crafted_engine(engine, B):
    ix, _ = crafted_db()
    e = engine()
    e.upload_index(ix, 0)
    reads = e.upload_fastx(B.text(), B.slots, view=True, keep=True)
    assert reads.count == len(B.reads)
    e.import_state(B.records())
    return e, reads, {key: ix for key in KEYS}


# ------------------------------------------------------------------------------------------------ 1. the sort seam
def sort_patterns(n, rng):
    yield "all equal", np.full(n, 5, dtype=np.uint32), 8
    yield "no pass", np.zeros(n, dtype=np.uint32), 0
    yield "below 256", rng.integers(0, 256, n).astype(np.uint32), 8
    yield "up to 2^16 + 5", rng.integers(0, 2 ** 16 + 6, n).astype(np.uint32), 17
    yield "up to 2^24 - 1", rng.integers(0, 2 ** 24, n).astype(np.uint32), 24
    yield "four passes", rng.integers(0, 2 ** 24, n).astype(np.uint32), 32
    hot = rng.integers(0, 70000, n).astype(np.uint32)
    hot[rng.random(n) < 0.99] = 4242
    yield "one key holds 99 %", hot, 17


def sort_body(engine, ns=SORT_NS):
    e = engine()
    rng = np.random.Generator(np.random.PCG64(5))
    try:
        for n in ns:
            for what, keys, bits in sort_patterns(n, rng):
                perm = e.otu_sort_batch(keys, bits)
                want = np.argsort(keys, kind="stable").astype(np.uint32)
                assert perm.shape == want.shape and (perm == want).all(), "n = %d, %s" % (n, what)
        for bad in ((np.asarray([256], dtype=np.uint32), 8), (np.asarray([1], dtype=np.uint32), 33)):
            try:
                e.otu_sort_batch(*bad)
                raise AssertionError("a key of more than key_bits bits must be refused")
            except smr.SmrError as x:
                assert "rc=-1" in str(x), x
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 2. crafted state
def crafted_body(engine, n_pairs, shape, fastq, tmp_path, seed=1):
    B = craft(n_pairs, shape, fastq, seed)
    e, reads, reg = crafted_engine(engine, B)
    try:
        before = e.export_records()
        run_pass(e, reg, lambda key: smr.default_params(), 0.9, 0.4)
        recs = e.export_records()
        host = host_report(tmp_path / "host", reads, recs, fastq, reg, 0.9, 0.4)
        res = {}
        dev = device_report(tmp_path / "dev", e, fastq, reg, lambda key: smr.default_params(), 0.9, 0.4, results=res)
        what = "%d pairs, %s, fastq=%s" % (n_pairs, shape, fastq)
        assert dev[0] == host[0], "%s: otu_map.txt differs" % what
        assert dev[1] == host[1], "%s: the number of groups differs" % what
        assert dev[2] == host[2], "%s: aligned_denovo differs" % what
        members = sum(int(g["n_reads"]) for key in res for g in res[key][1])
        assert members == n_pairs, "%s: the batch was crafted for %d members, the device found %d" % (what, n_pairs, members)
        assert all(res[key][2] == (n_pairs > 0) for key in res)
        n_groups = sum(len(res[key][1]) for key in res)
        if shape == "one" and n_pairs:
            assert n_groups == 1
        if shape == "own":
            assert n_groups == n_pairs
        if shape == "mixed" and n_pairs >= 63:                      # every kind the batch is crafted for was produced -- and, the expectations below being the host writer's, went through it
            assert set(B.kinds) == ALL_KINDS, ALL_KINDS - set(B.kinds)
            ids = set()
            for data, groups, _ in res.values():                     # (groups lie back to back: cut at their offsets first)
                ends = [int(g["off"]) for g in groups[1:]] + [len(data)]
                for g, end in zip(groups, ends):
                    ids.update(data[int(g["off"]):end].split(b"\t"))
            first_id = lambda kind: B.reads[B.kinds[kind][0]][0].split(" ")[0].lstrip(">@").encode()      # (the first read of a kind has a plain id: r4, r5, r6, r13)
            for kind in ("strand 0, forward letters equal", "N against N", "more than 64 operations"):      # these pass, and so stand in the device's map
                assert first_id(kind) in ids, kind
            assert first_id("strand 0, a true reverse complement") not in ids
        if shape == "mixed" and n_pairs >= 1025:
            data = res[(0, 0)][0]
            ids = data.replace(b"\t", b"\n").split(b"\n")
            assert any(len(x) == 1 for x in ids) and any(len(x) > 4096 for x in ids)
            starts = np.cumsum([0] + [len(x) + 1 for x in ids])[:-1]
            assert {int(x) % 4 for x in starts} == {0, 1, 2, 3}
            assert any(int(g["n_reads"]) > 1 for g in res[(0, 0)][1])
        assert e.export_records() == recs and [r[:8] + r[24:] for r in recs if r] == [r[:8] + r[24:] for r in before if r]      # no stored state changed
    finally:
        e.close()
        reads.free()


# ------------------------------------------------------------------------------------------------ 3. the second rounding
def rounding_body(engine, tmp_path):
    """min_cov = 9 * 0.001 > 9 / 1000.0: nine perfect columns of a 1000-letter read pass under fill_otu_map2's `* 0.001` and fail under the pass's
    `/ 1000.0`.  The read's other alignment, full length and perfect, puts its c_yid_ycov above 0; both references are in the map"""
    thr = 9 * 0.001
    assert thr > 9 / 1000.0
    _, refs = crafted_db()
    B = Batch(False)
    s = refs[0][100:1100]
    B.add("long_read", s, [m_aln(0, 100, 1000, 0, 1000), m_aln(1, 0, 9, 0, 1000)])
    e, reads, reg = crafted_engine(engine, B)
    try:
        run_pass(e, reg, lambda key: smr.default_params(), thr, thr)
        assert e.idcov_counters()["n_yid_ycov"] == 1 and e.idcov_counters()["n_yid_ncov"] == 1       # the pass itself does not let the nine columns through
        recs = e.export_records()
        host = host_report(tmp_path / "host", reads, recs, False, reg, thr, thr)
        res = {}
        dev = device_report(tmp_path / "dev", e, False, reg, lambda key: smr.default_params(), thr, thr, results=res)
        assert host[0] == b"ref0000\tlong_read\nref0001\tlong_read\n"
        assert dev[0] == host[0] and dev[1] == host[1] == 2
        assert [int(g["ref_num"]) for g in res[(0, 0)][1]] == [0, 1]
    finally:
        e.close()
        reads.free()


# ------------------------------------------------------------------------------------------------ 4. a map that exists and is empty
def empty_map_body(engine, tmp_path):
    _, refs = crafted_db()
    B = Batch(True)
    for i in range(70):
        r = 10 + i
        s = list(refs[r][:100])
        s[50] = "ACGT"[("ACGT".index(s[50]) + 1) % 4]                # one mismatch: no read is perfect
        B.add("imperfect%d" % i, "".join(s), [m_aln(r, 0, 100, 0, 100)])
    e, reads, reg = crafted_engine(engine, B)
    try:
        run_pass(e, reg, lambda key: smr.default_params(), 0.5, 0.5)
        recs = e.export_records()
        host = host_report(tmp_path / "host", reads, recs, True, reg, 1.0, 1.0)
        res = {}
        dev = device_report(tmp_path / "dev", e, True, reg, lambda key: smr.default_params(), 1.0, 1.0, results=res)
        assert all(r[2] and len(r[1]) == 0 and r[0] == b"" for r in res.values())
        assert host[0] == b"" and dev[0] == b"" and dev[1] == host[1] == 0
    finally:
        e.close()
        reads.free()


# ------------------------------------------------------------------------------------------------ 5. the reference's files
def reference_files_body(engine, case_setup, case, tmp_path, mode=0):
    g = otu.load()[case]
    cs = case_setup(g["inputs"])
    data = open(golden.inputs(g["inputs"])[1], "rb").read()
    is_otu = "-otu_map" in g["options"]
    e = engine(mode)
    try:
        reads = e.upload_fastx(data, cs["slots"], view=True, keep=True)
        steps = cs["steps"]
        for j, (k, part, ix) in enumerate(steps):                     # every part stays resident in a slot of its own
            p = cs["plist"][k]
            p.index_num, p.part, p.is_last_index_part = k, part, int(j == len(steps) - 1)
            e.upload_index(ix, j)
            e.align_part(j, p)
            e.traceback(j, p)
        reg = {(k, part): ix for k, part, ix in steps}
        slot = {(k, part): j for j, (k, part, ix) in enumerate(steps)}
        run_pass(e, reg, lambda key: cs["plist"][key[0]], g["min_id"], g["min_cov"], slot_of=lambda key: slot[key])
        recs = e.export_records()
        assert recs == otu.records(case)
        out = tmp_path / "dev"
        os.makedirs(str(out))
        rep = report.Report(str(out), is_fastq=False, fastx=False, other=False, otu_map=is_otu, denovo=True, min_id=g["min_id"], min_cov=g["min_cov"])
        for key, ix in reg.items():
            rep.set_part(key[0], key[1], ix)
        rep.skip_otu()
        rep.skip_denovo()
        if is_otu:
            for key, ix in reg.items():
                p = cs["plist"][key[0]]
                p.index_num, p.part = key
                d, groups, any_ = e.otu_part(slot[key], p, ix, g["min_id"], g["min_cov"])
                check_groups(d, groups)
                rep.add_otu(key[0], key[1], d, groups, any_)
        rep.add_denovo(e.fastx_denovo())
        for i, rec in enumerate(recs):                                # the per-read loop still runs and, with both switches on, adds nothing to either
            rep.add(*reads.record_text(i), rec)
        rep.close()
        assert rep.total_otu == g["n_groups"]
        assert (map_file(out) is not None) == (g["otu_map"] is not None)
        if g["otu_map"]:
            assert map_file(out) == open(os.path.join(otu.OTU_DIR, g["otu_map"]), "rb").read(), "%s: otu_map.txt differs from the reference's" % case
        assert denovo_files(out, False)[0] == open(os.path.join(otu.OTU_DIR, case + ".denovo.fa"), "rb").read(), "%s: aligned_denovo.fa differs from the reference's" % case
        assert e.export_records() == recs
        reads.free()
    finally:
        e.close()


PAIRED = ["paired_plain", "paired_in", "paired_out2", "paired_sout", "paired_out2_sout", "paired_loose", "paired_loose_in"]


def paired_body(engine, case, tmp_path):
    """the reference's paired fixture as ONE interleaved FASTQ batch (layout 1): its records after the pass, with the counters taken out, are
    imported; the pass puts the counters back (the records then equal the reference's again); the device's map and aligned_denovo.* streams
    must give the files the host writer gives from the same records, and the ids the reference wrote into each aligned_denovo file"""
    from . import fastx, paths, refrun
    g = otu.load()[case]
    m1 = fastx.read_fastx(os.path.join(paths.GOLDEN, "paired", "paired_1.fastq"))
    m2 = fastx.read_fastx(os.path.join(paths.GOLDEN, "paired", "paired_2.fastq"))
    want = otu.records(case)
    text = "".join("%s\n%s\n+\n%s\n" % r for pair in zip(m1, m2) for r in pair).encode()
    opt = dict(paired_in="-paired_in" in g["options"], out2="-out2" in g["options"], sout="-sout" in g["options"])
    parts = smr.Index.build(os.path.join(paths.GOLDEN, "real_db.fasta"), 18, 3072.0, 10000, 0)
    reg = {(0, j): ix for j, ix in enumerate(parts)}
    slots = max([len(refrun.parse_record(r)["alignv"]) for r in want if r] + [1])
    e = engine()
    try:
        for j, ix in enumerate(parts):
            e.upload_index(ix, j)
        reads = e.upload_fastx(text, slots, view=True, keep=True)
        assert reads.count == len(want) == 2 * len(m1)
        e.import_state([r[:8] + bytes(16) + r[24:] if r else r for r in want])
        run_pass(e, reg, lambda key: smr.default_params(), g["min_id"], g["min_cov"], slot_of=lambda key: key[1])
        recs = e.export_records()
        assert recs == want
        host = open_report(tmp_path / "host", True, reg, g["min_id"], g["min_cov"], **opt)
        dev = open_report(tmp_path / "dev", True, reg, g["min_id"], g["min_cov"], **opt)
        dev.skip_otu()
        dev.skip_denovo()
        for i in range(len(m1)):
            a, b = reads.record_text(2 * i) + (recs[2 * i],), reads.record_text(2 * i + 1) + (recs[2 * i + 1],)
            host.add_pair(a, b)
            dev.add_pair(a, b)
        for key, ix in reg.items():
            p = smr.default_params()
            p.index_num, p.part = key
            d, groups, any_ = e.otu_part(key[1], p, ix, g["min_id"], g["min_cov"])
            check_groups(d, groups)
            dev.add_otu(key[0], key[1], d, groups, any_)
        dev.add_denovo(e.fastx_denovo(layout=1, **opt))
        host.close()
        dev.close()
        reads.free()
    finally:
        e.close()
        for ix in parts:
            ix.free()
    names = sorted(os.listdir(str(tmp_path / "host")))
    assert names == sorted(os.listdir(str(tmp_path / "dev"))) and ("otu_map.txt" in names) == g["otu_map_exists"]
    for fn in names:
        assert open(tmp_path / "dev" / fn, "rb").read() == open(tmp_path / "host" / fn, "rb").read(), "%s: %s differs from the host writer's" % (case, fn)
    got = {fn: [l.split()[0][1:] for l in open(tmp_path / "dev" / fn).readlines()[0::4]] for fn in names if fn.startswith("aligned_denovo")}
    assert got == g["denovo_files"]
    assert dev.total_otu == host.total_otu


# ------------------------------------------------------------------------------------------------ 6. the routing of aligned_denovo.*
SUFFIXES = {1: ("",), "out2": ("_fwd", "_rev"), "sout": ("_paired", "_singleton"), 4: ("_paired_fwd", "_paired_rev", "_singleton_fwd", "_singleton_rev")}


def suffixes(o):
    n = fxsplit.num_out(o)
    return SUFFIXES[n] if n != 2 else SUFFIXES["out2" if o.get("out2") else "sout"]


def dn_record(is_dn):
    """a record whose counters make the read a de novo read (n_denovo = 1, the others 0) or not (c_yid_ycov = 1)"""
    r = bytearray(rows.record([m_aln(5, 0, 30, 0, 30)], 1))
    r[8:24] = struct.pack("<4I", 0, 0, 0, 1) if is_dn else struct.pack("<4I", 1, 0, 0, 0)
    return bytes(r)


def routing_text(fastq, n, tag):
    out = []
    for i in range(n):
        s = "ACGTTGCAAC" * 3 + "ACGT"[i % 4] * (i + 1)
        out.append(("@%s%d mate\n%s\n+\n%s\n" % (tag, i, s, "I" * len(s))) if fastq else (">%s%d mate\n%s\n" % (tag, i, s)))
    return "".join(out).encode()


def routing_body(engine, tmp_path, fastq=False):
    e = engine()
    try:
        reads = e.upload_fastx(routing_text(fastq, 6, "r"), 1, view=True, keep=True)       # layouts 0 and 1
        e.select_batch(1)
        mates = e.upload_fastx(routing_text(fastq, 3, "m"), 1, view=True, keep=True)       # layout 2: the mates of ...
        e.select_batch(2)
        three = e.upload_fastx(routing_text(fastq, 3, "r"), 1, view=True, keep=True)       # ... these
        n_case = 0
        for shift in range(4):
            combos = [(((shift + j) % 4) & 1, ((shift + j) % 4) >> 1) for j in range(3)]   # (dn of mate 1, of mate 2) of the three pairs: all four over the shifts
            for oi, o in enumerate(fxsplit.VALID_OPTS):
                for layout in (0, 1, 2):
                    d = tmp_path / ("%d_%d_%d" % (shift, oi, layout))
                    os.makedirs(str(d))
                    rep = report.Report(str(d), is_fastq=fastq, fastx=False, other=False, denovo=True, **(o if layout else {}))
                    if layout == 2:
                        dn = [c[0] for c in combos] + [c[1] for c in combos]
                        for k in range(3):
                            rep.add_pair(three.record_text(k) + (dn_record(dn[k]),), mates.record_text(k) + (dn_record(dn[3 + k]),))
                    else:
                        dn = [combos[i // 2][i % 2] for i in range(6)]
                        for k in range(3):
                            if layout == 1:
                                rep.add_pair(reads.record_text(2 * k) + (dn_record(dn[2 * k]),), reads.record_text(2 * k + 1) + (dn_record(dn[2 * k + 1]),))
                            else:
                                rep.add(*reads.record_text(2 * k), dn_record(dn[2 * k]))
                                rep.add(*reads.record_text(2 * k + 1), dn_record(dn[2 * k + 1]))
                    rep.close()
                    sfx = suffixes(o) if layout else ("",)
                    want = [x or b"" for x in denovo_files(d, fastq, sfx)] + [b""] * (4 - len(sfx))
                    e.select_batch(2 if layout == 2 else 0)
                    got = e.fastx_denovo(layout=layout, mates=1 if layout == 2 else None, dn=dn, **(o if layout else {}))
                    assert got == want, "dn %s, %s, layout %d" % (dn, fxsplit.opts_id(o), layout)
                    n_case += 1
        assert n_case == 4 * 8 * 3
        # without the override and without the pass: no de novo read
        assert e.fastx_denovo() == [b""] * 4
        for r in (reads, mates, three):
            r.free()
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 7. the contract
def call(e, slot, p, ix, min_id, min_cov, buf, cap, groups, gcap):
    need = (C.c_uint64 * 2)(9, 9)
    any_ = C.c_int(9)
    rc = e.L.smr_otu_part(e.h, slot, C.byref(p), ix.h, min_id, min_cov, buf.ctypes.data if buf is not None else None, cap,
                          groups.ctypes.data if groups is not None else None, gcap, need, C.byref(any_))
    return rc, list(need), any_.value


def contract_body(engine, tmp_path):
    ix, refs = crafted_db()
    B = craft(130, "mixed", True, seed=9)
    e, reads, reg = crafted_engine(engine, B)
    p = smr.default_params()
    G = smr.engine.OTU_GROUP
    try:
        # a batch on which the pass never ran: no error, nothing
        assert call(e, 0, p, ix, 0.9, 0.4, None, 0, None, 0) == (0, [0, 0], 0)
        run_pass(e, reg, lambda key: smr.default_params(), 0.9, 0.4)
        e.fetch()
        before = e.records()
        recs = e.export_records()
        # sizes only
        rc, need, any_ = call(e, 0, p, ix, 0.9, 0.4, None, 0, None, 0)
        assert rc == 0 and need[0] > 0 and need[1] > 0 and any_ == 1
        buf = np.full(need[0] + 64, 0x5A, dtype=np.uint8)
        grp = np.zeros(need[1] + 4, dtype=G)
        grp.view(np.uint8)[:] = 0x5A
        # one short in either: refused, nothing written, the sizes valid
        for cap, gcap in ((need[0] - 1, need[1]), (need[0], need[1] - 1)):
            rc, need2, _ = call(e, 0, p, ix, 0.9, 0.4, buf, cap, grp, gcap)
            assert rc == ERR_CAPACITY and need2 == need and (buf == 0x5A).all() and (grp.view(np.uint8) == 0x5A).all()
        # exactly the sizes: nothing behind them
        rc, need2, _ = call(e, 0, p, ix, 0.9, 0.4, buf, need[0], grp, need[1])
        assert rc == 0 and need2 == need and (buf[need[0]:] == 0x5A).all() and (grp[need[1]:].view(np.uint8) == 0x5A).all()
        first, first_g = buf[:need[0]].tobytes(), grp[:need[1]].tobytes()
        check_groups(first, grp[:need[1]])
        # again: the same
        buf[:] = 0x5A
        grp.view(np.uint8)[:] = 0x5A
        assert call(e, 0, p, ix, 0.9, 0.4, buf, len(buf), grp, len(grp))[0] == 0
        assert buf[:need[0]].tobytes() == first and grp[:need[1]].tobytes() == first_g and (buf[need[0]:] == 0x5A).all()
        e.fetch()
        assert e.records() == before                                 # stored records unchanged
        buf[:] = 0x5A
        grp.view(np.uint8)[:] = 0x5A
        full = (buf, len(buf), grp, len(grp))
        # thresholds
        for bad in ((1.5, 0.5), (0.5, -0.1), (float("nan"), 0.5)):
            assert call(e, 0, p, ix, *bad, *full)[0] == ERR_ARG and "smr_otu_part" in e.L.smr_last_error(e.h).decode()
        # not the part in the slot
        other = smr.Index.build(golden.inputs("t9")[0], 18, 3072.0, 10000, 0)[0]
        assert call(e, 0, p, other, 0.9, 0.4, *full)[0] == ERR_ARG and "slot" in e.L.smr_last_error(e.h).decode()
        other.free()
        assert call(e, 0, p, ix, 0.9, 0.4, *full)[0] == 0
        buf[:] = 0x5A
        grp.view(np.uint8)[:] = 0x5A
        # what the host writer would refuse.  The bad alignment belongs to key (1, 0), on which the pass is not run here (it would walk it);
        # the read's good alignment of key (0, 0) puts its c_yid_ycov above 0.  In a read whose counter is 0 the same alignment is not looked at
        s = refs[20][:100]
        good, cold = m_aln(20, 0, 100, 0, 100), m_aln(21, 0, 100, 0, 100)
        bad_sets = {"a CIGAR past its read": (dict(good, cigar=[(101 << 4) | 0]), ERR_ARG),
                    "a CIGAR past its reference": (dict(good, ref_begin1=len(refs[20]) - 99), ERR_ARG),
                    "a negative start": (dict(good, read_begin1=-1), ERR_ARG),
                    "ref_num beyond the part": (dict(good, ref_num=N_REFS), ERR_ARG),
                    "no CIGAR": (dict(good, cigar=[]), ERR_STATE),
                    # insertions or deletions that alone run past the end: no M column lies outside, the host writer accepts it, so does the device
                    "an insertion past the read": (dict(good, cigar=[(100 << 4) | 0, (5 << 4) | 1]), 0),
                    "a deletion past the reference": (dict(good, ref_begin1=len(refs[20]) - 100, cigar=[(100 << 4) | 0, (5 << 4) | 2]), 0)}
        B2 = Batch(True)
        B2.add("guard", s, [])
        B2.add("cold", "ACGT" * 25, [])
        e.select_batch(1)
        r2 = e.upload_fastx(B2.text(), B2.slots, view=True, keep=True)
        p1 = smr.default_params()
        p1.index_num = 1
        for what, (aln, want_rc) in bad_sets.items():
            bad = dict(aln, index_num=1)
            for hot in (False, True):
                e.reset_state()
                e.import_state([rows.record([good] + ([bad] if hot else []), B2.slots), rows.record([cold, bad], B2.slots)])
                run_pass(e, {(0, 0): ix}, lambda key: smr.default_params(), 0.9, 0.4)
                assert e.idcov_counters()["n_yid_ycov"] == 1
                rc, need3, any3 = call(e, 0, p1, ix, 0.9, 0.4, *full)
                if hot:
                    assert rc == want_rc, (what, rc, e.L.smr_last_error(e.h).decode())
                    if want_rc == 0:                                 # (accepted: it passes and is written; the host writer takes the same records)
                        tmp = tmp_path / ("ok_%d" % len(what))             # the host writer takes the same records without an error, and finds as many members
                        host_map = host_report(tmp, r2, e.export_records(), True, {(0, 0): ix, (1, 0): ix}, 0.9, 0.4)[0]
                        assert host_map.count(b"guard") == 1 + need3[1] and need3[0] == need3[1] * len(b"guard"), (what, need3, host_map)
                        assert need3[1] == (1 if "insertion" in what else 0)      # (the deletion's window does not hold the read's letters: it fails %id, on both sides)
                        buf[:] = 0x5A
                        grp.view(np.uint8)[:] = 0x5A
                        continue
                    assert "smr_otu_part" in e.L.smr_last_error(e.h).decode(), what
                else:
                    assert (rc, need3, any3) == (0, [0, 0], 1), (what, rc, need3, any3)
                assert (buf == 0x5A).all() and (grp.view(np.uint8) == 0x5A).all(), what
        r2.free()
        # a batch without kept text
        plain = smr.Reads.from_seqs([reads.record_text(i)[1] for i in range(reads.count)])
        e.upload_reads(plain, B.slots)
        e.import_state(B.records())
        assert call(e, 0, p, ix, 0.9, 0.4, *full)[0] == ERR_STATE and "SMR_FASTX_KEEP" in e.L.smr_last_error(e.h).decode()
        off = (C.c_uint64 * 5)()
        o = smr.capi.FxSplitOpts(0, 0, 0, 0, 0, 1, 1)
        assert e.L.smr_fastx_denovo(e.h, -1, C.byref(o), None, None, 0, off, None) == ERR_STATE and "SMR_FASTX_KEEP" in e.L.smr_last_error(e.h).decode()
        assert (buf == 0x5A).all()
        plain.free()
        e.select_batch(0)
        # the context goes on working
        assert call(e, 0, p, ix, 0.9, 0.4, *full)[0] == 0 and buf[:need[0]].tobytes() == first and grp[:need[1]].tobytes() == first_g
        assert e.export_records() == recs
    finally:
        e.close()
        reads.free()


# ------------------------------------------------------------------------------------------------ the report side
def report_side_body(tmp_path):
    ix, _ = crafted_db()
    G = smr.engine.OTU_GROUP
    os.makedirs(str(tmp_path / "a"))
    rep = report.Report(str(tmp_path / "a"), is_fastq=False, fastx=False, other=False, otu_map=True, denovo=True)
    rep.set_part(0, 0, ix)
    try:
        def add(data, gl, key=(0, 0), r=rep):
            g = np.asarray(gl, dtype=G)
            return r.L.smr_report_add_otu(r.h, key[0], key[1], data, len(data), g.ctypes.data if len(g) else None, len(g), 1)
        assert add(b"a\tb", [(1, 2, 0)], key=(0, 1)) == ERR_ARG                   # not registered
        assert add(b"a\tbc", [(1, 2, 3), (2, 1, 2)]) == ERR_ARG                   # offsets decrease
        assert add(b"a\tbc", [(1, 2, 0), (2, 1, 9)]) == ERR_ARG                   # past the bytes
        assert add(b"a\tbc", [(1, 0, 0)]) == ERR_ARG                              # a group without members
        assert add(b"a\tbc", [(1, 2, 0), (2, 3, 3)]) == ERR_ARG                   # fewer ids than members (and nothing of the first group was appended)
        assert add(b"a\tbc", [(1, 2, 0), (N_REFS + 5, 1, 3)]) == 0
        assert add(b"d", [(1, 1, 0)]) == 0                                        # behind what the key holds
        assert add(b"ef", [(N_REFS + 6, 1, 0), (N_REFS + 7, 1, 1)]) == 0        # two more references beyond the table: all print "*", appended reference after reference
        off = (C.c_uint64 * 5)
        assert rep.L.smr_report_add_denovo(rep.h, b">x\nAC\n", off(0, 6, 6, 5, 6)) == ERR_ARG      # offsets decrease
        assert rep.L.smr_report_add_denovo(rep.h, b">x\nAC\n", off(0, 0, 6, 6, 6)) == ERR_ARG      # no such file
        assert rep.L.smr_report_add_denovo(rep.h, b">x\nAC\n", off(0, 6, 6, 6, 6)) == 0
    finally:
        rep.close()
    assert rep.total_otu == 2
    assert map_file(tmp_path / "a") == b"*\tc\te\tf\nref0001\ta\tb\td\n"
    assert denovo_files(tmp_path / "a", False)[0] == b">x\nAC\n"
    os.makedirs(str(tmp_path / "b"))
    rep = report.Report(str(tmp_path / "b"), is_fastq=False, fastx=False, other=False)
    rep.set_part(0, 0, ix)
    try:
        g = np.asarray([(1, 1, 0)], dtype=G)
        assert rep.L.smr_report_add_otu(rep.h, 0, 0, b"a", 1, g.ctypes.data, 1, 1) == ERR_ARG      # opened without otu_map
    finally:
        rep.close()
