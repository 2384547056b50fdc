"""The fixtures of the %id / %coverage pass (tests/golden/otu/, written by tests/golden/make_golden_otu.py from the unmodified
reference) and the test bodies that the emulator suite and the GPU suite share.  TEST INFRASTRUCTURE ONLY."""
import json
import os
import struct

import numpy as np

import sortmerna_amd as smr

from . import cases, golden, paths

OTU_DIR = os.path.join(paths.GOLDEN, "otu")
_G = None


def load():
    global _G
    if _G is None:
        _G = json.load(open(os.path.join(OTU_DIR, "otu.json")))
    return _G


def records(case):
    d = open(os.path.join(OTU_DIR, load()[case]["records"]), "rb").read()
    (n,) = struct.unpack_from("<I", d, 0)
    o = 4
    out = []
    for _ in range(n):
        (l,) = struct.unpack_from("<I", d, o)
        o += 4
        out.append(d[o:o + l])
        o += l
    return out


def run(engine, case, tmpdir, id_cov=True):
    """align -> traceback -> idcov_part per (index, part) of a fixture case; -> (records, totals dict, what is needed to call again)"""
    g = load()[case]
    src = g["inputs"]
    idx, seqs = cases.build_case(src, tmpdir)
    gp = golden.load()[src]["params"]
    params = {k: v for k, v in gp.items() if k not in ("max_mb", "evalue", "lnwin")}
    reads = smr.Reads.from_seqs(seqs)
    plist = [smr.default_params(minimal_score=d["minimal_score"], **params) for d in idx]
    slots = 256 if plist[0].num_alignments == 0 else None
    smr.align(engine, reads, [d["parts"] for d in idx], plist, with_cigar=True, max_alignments_per_read=slots,
              id_cov=(g["min_id"], g["min_cov"]) if id_cov else None)
    return engine.records(), engine.idcov_counters(), (idx, plist, reads)


def free(keep):
    idx, _, reads = keep
    reads.free()
    for d in idx:
        for ix in d["parts"]:
            ix.free()


def body_records_and_totals(engine, case, tmpdir):
    """records after the pass == the reference's records after denovo_stats, byte for byte; the four totals equal; a second call of the
    pass changes nothing"""
    g = load()[case]
    want = records(case)
    got, tot, keep = run(engine, case, tmpdir)
    try:
        bad = [i for i in range(len(want)) if want[i] != got[i]]
        assert not bad, "%s: %d of %d records differ from the reference's after denovo_stats (first: read %d)" % (case, len(bad), len(want), bad[0])
        assert [tot["n_yid_ycov"], tot["n_yid_ncov"], tot["n_nid_ycov"], tot["num_denovo"]] == g["totals"]
        idx, plist, _ = keep
        for k, d in enumerate(idx):
            for part, ix in enumerate(d["parts"]):
                p = plist[k]
                p.index_num, p.part = k, part
                engine.upload_index(ix, 0)
                engine.idcov_part(0, p, g["min_id"], g["min_cov"])
                engine.unload_index(0)
        engine.fetch()
        assert engine.idcov_counters() == tot
        assert engine.records() == got
    finally:
        free(keep)


def body_without_the_pass_the_counters_are_zero(engine, case, tmpdir):
    got, tot, keep = run(engine, case, tmpdir, id_cov=False)
    free(keep)
    assert tot == dict(n_yid_ycov=0, n_yid_ncov=0, n_nid_ycov=0, num_denovo=0)
    assert got == golden.records(load()[case]["inputs"])


def body_pass_before_traceback_is_a_state_error(engine, case, tmpdir):
    g = load()[case]
    idx, seqs = cases.build_case(g["inputs"], tmpdir)
    reads = smr.Reads.from_seqs(seqs)
    p = smr.default_params(minimal_score=idx[0]["minimal_score"])
    p.index_num, p.part, p.is_last_index_part = 0, 0, 1
    try:
        engine.upload_reads(reads, 1)
        engine.upload_index(idx[0]["parts"][0], 0)
        engine.align_part(0, p)
        try:
            engine.idcov_part(0, p, 0.97, 0.97)
            raise AssertionError("smr_idcov_part before smr_traceback must fail")
        except smr.SmrError as e:
            assert "rc=-5" in str(e), e                  # SMR_ERR_STATE
        assert engine.idcov_counters() == dict(n_yid_ycov=0, n_yid_ncov=0, n_nid_ycov=0, num_denovo=0)
        for bad in ((1.5, 0.5), (0.5, -0.1), (float("nan"), 0.5)):
            try:
                engine.idcov_part(0, p, *bad)
                raise AssertionError("thresholds outside [0, 1] must be refused")
            except smr.SmrError as e:
                assert "rc=-1" in str(e), e              # SMR_ERR_ARG
        engine.traceback(0, p)
        engine.idcov_part(0, p, 0.97, 0.97)
        assert sum(engine.idcov_counters().values()) > 0
        try:
            engine.align_part(0, p)
            raise AssertionError("smr_align_part after the pass must fail until the state is reset")
        except smr.SmrError as e:
            assert "rc=-5" in str(e), e
        engine.reset_state()
        assert engine.idcov_counters() == dict(n_yid_ycov=0, n_yid_ncov=0, n_nid_ycov=0, num_denovo=0)
        engine.align_part(0, p)
        engine.unload_index(0)
    finally:
        reads.free()
        for d in idx:
            for ix in d["parts"]:
                ix.free()


# ---- the seam smr_idcov_batch ----------------------------------------------------------------------------------------------------------

def host_counts(read, ref, cigar, read_begin):
    """Read::calc_miss_gap_match (read.cpp:547-589) in plain Python"""
    pb, qb, miss, gap, match = read_begin, 0, 0, 0, 0
    for c in cigar:
        op, ln = int(c) & 15, int(c) >> 4
        if op == 0:
            a = np.frombuffer(bytes(read[pb:pb + ln]), dtype=np.uint8)
            b = np.frombuffer(bytes(ref[qb:qb + ln]), dtype=np.uint8)
            m = int((a == b).sum())
            match += m
            miss += ln - m
            pb += ln
            qb += ln
        elif op == 1:
            pb += ln
            gap += ln
        else:
            qb += ln
            gap += ln
    return miss, gap, match


def host_class(miss, gap, match, read_begin, read_end, readlen, min_id, min_cov):
    """the decision of denovo_stats_run (processor.cpp:334-355) in Python floats: IEEE doubles, every operation rounded on its own"""
    import math
    tot = miss + gap + match
    idf = float(match) / float(tot)
    cov = float(abs(read_end - read_begin + 1)) / float(readlen)
    idr = math.floor(idf * 1000.0 + 0.5) / 1000.0
    covr = math.floor(cov * 1000.0 + 0.5) / 1000.0
    is_id, is_cov = idr >= min_id, covr >= min_cov
    return 0 if (is_id and is_cov) else 1 if is_id else 2 if is_cov else 3


def handmade_triples():
    """-> (reads, refs, cigars, read_begin, read_end, readlen): CIGARs of more than 64 operations, runs that cross the packed words of the
    read (16 letters per code word, 32 per mask word) and the dwords of the reference at every alignment, ambiguous letters on both sides"""
    rng = np.random.Generator(np.random.PCG64(2024))
    M, I, D = 0, 1, 2
    T = []

    def add(read, ref, cig, rb):
        read, ref = np.asarray(read, dtype=np.uint8), np.asarray(ref, dtype=np.uint8)
        span = sum(c >> 4 for c in cig if (c & 15) != D)
        T.append((read.tobytes(), ref.tobytes(), np.asarray(cig, dtype=np.uint32), rb, rb + span - 1, len(read)))

    def op(ln, o):
        return (ln << 4) | o
    # an ambiguous read letter (4) against a reference N (4): a match; against A: a mismatch; a read A against N: a mismatch
    add([4, 4, 0, 1, 2], [4, 0, 4, 1, 2], [op(5, M)], 0)
    # one run starting at every offset within a code word / mask word, the window at every byte alignment, lengths around 16, 32, 64
    for rb in (0, 1, 15, 16, 17, 31, 32, 33):
        for ln in (1, 15, 16, 17, 31, 33, 64, 65, 150):
            read = rng.integers(0, 4, size=rb + ln + 3)
            read[rng.random(len(read)) < 0.05] = 4
            ref = read[rb:rb + ln].copy()
            flip = rng.random(ln) < 0.2
            ref[flip] = (ref[flip] + 1) % 5
            add(read, ref, [op(ln, M)], rb)
    # several windows back to back, so that reference windows start at every alignment modulo 4 (lengths 1, 2, 3 shift what follows)
    for ln in (1, 2, 3, 5, 6, 7):
        read = rng.integers(0, 4, size=ln)
        add(read, read.copy(), [op(ln, M)], 0)
    # a few operations with gaps (k_idcov_few) and hundreds of short ones (k_idcov_many: 65, 128, 129, 700 operations)
    for nops in (3, 7, 8, 9, 64, 65, 128, 129, 700):
        cig, read, ref = [], [], []
        for q in range(nops):
            o = M if q % 2 == 0 else (I if (q // 2) % 2 == 0 else D)
            ln = int(rng.integers(1, 24)) if o == M else int(rng.integers(1, 4))
            cig.append(op(ln, o))
            if o == M:
                seg = rng.integers(0, 5, size=ln)
                r2 = seg.copy()
                flip = rng.random(ln) < 0.15
                r2[flip] = (r2[flip] + 2) % 5
                read += list(seg)
                ref += list(r2)
            elif o == I:
                read += list(rng.integers(0, 4, size=ln))
            else:
                ref += list(rng.integers(0, 4, size=ln))
        lead = int(rng.integers(0, 40))
        add(list(rng.integers(0, 4, size=lead)) + read + [1, 2], ref, cig, lead)
    return tuple(list(x) for x in zip(*T))


def body_handmade_triples(engine):
    reads, refs, cigars, rb, re_, rl = handmade_triples()
    for thr in ((0.97, 0.97), (0.5, 0.9), (0.0, 0.0), (1.0, 1.0)):
        out = engine.idcov_batch(reads, refs, cigars, rb, re_, rl, *thr)
        for i in range(len(reads)):
            want = host_counts(reads[i], refs[i], cigars[i], rb[i])
            assert tuple(int(x) for x in out[i][:3]) == want, (i, out[i], want)
            assert int(out[i][3]) == host_class(*want, rb[i], re_[i], rl[i], *thr), (i, thr, out[i])
    # the first triple, spelled out: read N N A C G against reference N A N C G
    assert tuple(int(x) for x in engine.idcov_batch(reads[:1], refs[:1], cigars[:1], rb[:1], re_[:1], rl[:1], 0.5, 0.5)[0]) == (2, 0, 3, 0)
    # a CIGAR that runs past its read is refused, not walked
    try:
        engine.idcov_batch([b"\x00\x01"], [b"\x00\x01\x02"], [np.asarray([3 << 4], dtype=np.uint32)], [0], [2], [2], 0.5, 0.5)
        raise AssertionError("a CIGAR longer than its read must be refused")
    except smr.SmrError as e:
        assert "rc=-1" in str(e), e


def body_accumulate_carries_the_four_sums(engine, tmpdir, device_zeros, to_host):
    """two batches (the fixture cases syn and two_db) summed on the device: k < 66 as before, k = 66 .. 69 the four sums of the pass.
    device_zeros(n) -> (object that owns n u64 zeros in device memory, its address); to_host(object) -> list of ints"""
    acc, addr = device_zeros(70)
    want = [0, 0, 0, 0]
    aligned = 0
    for case in ("syn", "two_db"):
        _, tot, keep = run(engine, case, tmpdir)
        free(keep)
        assert [tot["n_yid_ycov"], tot["n_yid_ncov"], tot["n_nid_ycov"], tot["num_denovo"]] == load()[case]["totals"]
        aligned += engine.counters(1)["num_aligned"]
        for k, v in enumerate(load()[case]["totals"]):
            want[k] += v
        engine.counters_accumulate(addr, 70)
    h = to_host(acc)
    assert h[66:70] == want and h[0] == aligned, (h[:4], h[66:70], want, aligned)
    try:
        engine.counters_accumulate(addr, 71)
        raise AssertionError("more than 70 counters must be refused")
    except smr.SmrError as e:
        assert "rc=-1" in str(e), e


def long_read_triples(engine, tmpdir, n_reads=40, read_len=5000):
    """a 5 kb noisy long-read workload through align + traceback: every stored alignment as a triple for the seam (the FORWARD read, the
    reference window from ref_begin1 on, its CIGAR)"""
    from sortmerna_amd import synth
    from .workload import Workload
    from . import refrun
    w = Workload(str(tmpdir), db_nt=400_000, n_reads=n_reads, read_len=read_len, frac_db=0.9, seed=77, family_size=4, mean_len=9000,
                 read_kw=dict(sub=0.05, indel=0.05))
    recs, _ = w.gpu_records(engine, num_alignments=2)
    codes, offs = synth.load_db_codes(w.db)
    lut = np.full(256, 4, dtype=np.uint8)
    for i, c in enumerate(b"ACGT"):
        lut[c] = i
        lut[ord(chr(c).lower())] = i
    lut[ord("U")] = lut[ord("u")] = 3
    T = []
    for i, r in enumerate(recs):
        f = refrun.parse_record(r)
        if not f:
            continue
        read = lut[np.frombuffer(w.seqs[i].encode(), dtype=np.uint8)]
        for a in f["alignv"]:
            ref = codes[offs[a["ref_num"]] + a["ref_begin1"]: offs[a["ref_num"]] + a["ref_end1"] + 1]
            T.append((read.tobytes(), ref.tobytes(), np.asarray(a["cigar"], dtype=np.uint32), a["read_begin1"], a["read_end1"], a["readlen"]))
    for ix in w.parts:
        ix.free()
    w.reads.free()
    return tuple(list(x) for x in zip(*T))


def body_long_reads(engine, tmpdir, n_reads=40, min_ops=129):       # min_ops: at least three rounds of 64 operations in k_idcov_many
    reads, refs, cigars, rb, re_, rl = long_read_triples(engine, tmpdir, n_reads)
    assert len(reads) >= n_reads // 2 and max(len(c) for c in cigars) >= min_ops, (len(reads), max(len(c) for c in cigars))
    out = engine.idcov_batch(reads, refs, cigars, rb, re_, rl, 0.9, 0.9)
    classes = set()
    for i in range(len(reads)):
        want = host_counts(reads[i], refs[i], cigars[i], rb[i])
        assert tuple(int(x) for x in out[i][:3]) == want, (i, out[i], want)
        assert int(out[i][3]) == host_class(*want, rb[i], re_[i], rl[i], 0.9, 0.9), (i, out[i])
        classes.add(int(out[i][3]))
    return classes


# ---- the arithmetic of the decision -----------------------------------------------------------------------------------------------------
THRESHOLDS = (0.0, 0.5, 0.9, 0.9695, 0.97, 1.0)


def arithmetic_triples(n_tots):
    """one synthetic triple per (n_tot, n_match <= n_tot): n_tot aligned columns of which n_match are equal (read all A; reference A then C)"""
    reads, refs, cigars, rb, re_, rl, nm = [], [], [], [], [], [], []
    for n_tot in n_tots:
        read = bytes(n_tot)
        cig = np.asarray([n_tot << 4], dtype=np.uint32)
        for n_match in range(n_tot + 1):
            reads.append(read)
            refs.append(bytes(n_match) + b"\x01" * (n_tot - n_match))
            cigars.append(cig)
            rb.append(0)
            re_.append(n_tot - 1)
            rl.append(n_tot)
            nm.append(n_match)
    return reads, refs, cigars, rb, re_, rl, nm


def body_arithmetic(engine, n_tots, chunk=40000):
    reads, refs, cigars, rb, re_, rl, nm = arithmetic_triples(n_tots)
    n = len(reads)
    for thr in THRESHOLDS:
        for lo in range(0, n, chunk):
            hi = min(n, lo + chunk)
            out = engine.idcov_batch(reads[lo:hi], refs[lo:hi], cigars[lo:hi], rb[lo:hi], re_[lo:hi], rl[lo:hi], thr, thr)
            for i in range(lo, hi):
                o = out[i - lo]
                assert (int(o[0]), int(o[1]), int(o[2])) == (rl[i] - nm[i], 0, nm[i]), (i, o)
                assert int(o[3]) == host_class(rl[i] - nm[i], 0, nm[i], 0, rl[i] - 1, rl[i], thr, thr), (rl[i], nm[i], thr, int(o[3]))
    return n
