"""Two batches of mates and the host writer's answer for the tests of smr_otu_part_mates (test_gpu_otu_mates.py runs the bodies on the GPU,
test_emu_otu_mates.py on the kernel emulator).  TEST INFRASTRUCTURE ONLY.

The yardstick is always smr_report_add_pair (Report.add_pair): mate 1 of pair i is read i of batch 0, mate 2 read i of batch 1; both go through
it into a temporary directory with the records the pass left, and the otu_map.txt it wrote is compared with what smr_otu_part_mates +
smr_report_add_otu give in a report that skips its own map.  Builds on helpers/otu_device.py (the crafted database, Batch, m_aln, open_report,
check_groups, run_pass)."""
import ctypes as C
import os

import numpy as np

import sortmerna_amd as smr

from . import golden, otu, rows
from . import otu_device as od
from .matesdev import COUNTS                                  # noqa: F401  (1, 63, 64, 65, 255, 256, 257, 1025)

ERR_ARG, ERR_CAPACITY, ERR_STATE = od.ERR_ARG, od.ERR_CAPACITY, od.ERR_STATE
SHAPES = ["mixed", "one", "a only", "b only"]
KINDS = ["member of A only", "member of B only", "members of both", "mate 2 passes, mate 1 has no counter", "a counter and no passing slot of this key",
         "several slots on different references", "neither"]
MIN_ID, MIN_COV = 0.9, 0.4


# ------------------------------------------------------------------------------------------------ crafted pairs
def mate_header(i, long_at=None):
    """ids of batch B: another alphabet and other lengths than od.header_of gives batch A (r<i> ...), so that an id read from the wrong text, or
    placed by the wrong offset rule, changes the bytes"""
    if long_at is not None and i == long_at:
        return "LONGMATE%d_" % i + "z" * 5000 + " behind the id"      # longer than the 4 KB window
    return ["mate%d/2", "M%dyyyyyyyy words", "@m%d", "%dB two  blanks", "mt%d_a_longer_id_of_batch_b x"][i % 5] % i


def read_header(i):
    """ids of batch A: the forms of od.header_of without the one that holds a tab (the tests here cut the device's text at tabs)"""
    if i % 17 == 3:
        return "abcdefghij"[i % 10]                                 # an id of one byte
    return ["r%d", "r%d some words", ">r%d", "@r%d x", "r%d ", "r%d  two", "%d"][i % 7] % i


def craft_pairs(n, shape, fastq, seed=1, long_at=None):
    """-> (A, B, members): two od.Batch of n reads each, two alignment slots a read; members: how many the map of the two keys must hold.
    mixed: every kind of KINDS, twice over in the first pairs whatever the seed, then at random; one: every read of both batches twice in the
    group of reference 7 (4 n members in one group); a only / b only: one member a pair, all in that batch"""
    _, refs = od.crafted_db()
    rng = np.random.Generator(np.random.PCG64(seed))
    A, B = od.Batch(fastq, slots=2), od.Batch(fastq, slots=2)
    members = 0

    def piece(r, L=100):
        b = int(rng.integers(0, len(refs[r]) - L + 1))
        return b, refs[r][b:b + L]

    def passing(r=None, key=od.KEYS[0]):
        r = int(rng.integers(4, od.N_REFS)) if r is None else r
        b, s = piece(r)
        return s, [od.m_aln(r, b, 100, 0, 100, key=key)]

    def failing():                                              # random letters against a reference: c_yid_ycov stays 0
        return "".join("ACGT"[int(c)] for c in rng.integers(0, 4, 100)), [od.m_aln(int(rng.integers(4, od.N_REFS)), 2, 100, 0, 100)]

    def nothing():
        return "ACGTTGCA" * 10, []

    def two_refs():                                             # two halves on two different references
        r1 = int(rng.integers(4, od.N_REFS - 1)); r2 = r1 + 1
        (b1, s1), (b2, s2) = piece(r1, 50), piece(r2, 50)
        return s1 + s2, [od.m_aln(r2, b2, 50, 50, 100), od.m_aln(r1, b1, 50, 0, 100)]

    hot = int(rng.integers(4, od.N_REFS))                       # in `mixed`, a reference that takes members of both batches again and again
    for i in range(n):
        ha = read_header(i)
        hb = mate_header(i, long_at)
        if shape == "one":
            b, s = piece(7)
            two = [od.m_aln(7, b, 100, 0, 100), od.m_aln(7, b, 100, 0, 100)]
            A.add(ha, s, two); B.add(hb, s, two); members += 4
            continue
        if shape in ("a only", "b only"):
            s, al = passing()
            (A if shape == "a only" else B).add(ha if shape == "a only" else hb, s, al)
            (B if shape == "a only" else A).add(hb if shape == "a only" else ha, *nothing())
            members += 1
            continue
        k = i % len(KINDS) if i < 2 * len(KINDS) else int(rng.integers(0, len(KINDS)))
        r = hot if rng.integers(0, 3) == 0 else None
        if k == 0:
            A.add(ha, *passing(r)); B.add(hb, *nothing()); members += 1
        elif k == 1:
            A.add(ha, *nothing()); B.add(hb, *passing(r)); members += 1
        elif k == 2:
            A.add(ha, *passing(r)); B.add(hb, *passing(r)); members += 2
        elif k == 3:
            A.add(ha, *failing()); B.add(hb, *passing(r)); members += 1
        elif k == 4:                                            # the counter comes from key (1, 0): a member there, none under key (0, 0)
            A.add(ha, *passing(r, key=od.KEYS[1])); B.add(hb, *passing(r)); members += 2
        elif k == 5:
            A.add(ha, *two_refs()); B.add(hb, *two_refs()); members += 4
        else:
            A.add(ha, *failing()); B.add(hb, *nothing())
        A.mark(KINDS[k])
    return A, B, members


class Pair:
    """an engine with the crafted part in slot 0 and the batches A, B in batches 0 and 1 (records imported), batch 0 selected"""

    def __init__(self, engine, A, B):
        self.ix, _ = od.crafted_db()
        self.reg = {key: self.ix for key in od.KEYS}
        self.fastq = A.fastq
        self.e = engine()
        self.e.upload_index(self.ix, 0)
        self.reads = []
        for k, X in enumerate((A, B)):
            self.e.select_batch(k)
            self.reads.append(self.e.upload_fastx(X.text(), X.slots, view=True, keep=True))
            assert self.reads[k].count == len(X.reads)
            self.e.import_state(X.records())
        self.e.select_batch(0)

    def run_pass(self, min_id=MIN_ID, min_cov=MIN_COV, batches=(0, 1)):
        for k in batches:
            self.e.select_batch(k)
            od.run_pass(self.e, self.reg, lambda key: smr.default_params(), min_id, min_cov)
        self.e.select_batch(0)

    def records(self):
        out = []
        for k in (0, 1):
            self.e.select_batch(k)
            out.append(self.e.export_records())
        self.e.select_batch(0)
        return out

    def close(self):
        self.e.close()
        for r in self.reads:
            r.free()


def feed_pairs(rep, reads, recs):
    for i in range(len(recs[0])):
        rep.add_pair(reads[0].record_text(i) + (recs[0][i],), reads[1].record_text(i) + (recs[1][i],))


def host_map(tmpdir, reads, recs, fastq, reg, min_id=MIN_ID, min_cov=MIN_COV):
    """smr_report_add_pair over the pairs -> (otu_map.txt or None, total_otu)"""
    rep = od.open_report(tmpdir, fastq, reg, min_id, min_cov)
    feed_pairs(rep, reads, recs)
    rep.close()
    return od.map_file(tmpdir), rep.total_otu


def device_map(tmpdir, e, reads, recs, fastq, reg, min_id=MIN_ID, min_cov=MIN_COV, results=None):
    """skip_otu, smr_otu_part_mates per key + smr_report_add_otu; the pairs go through the report as well, which must add nothing to the map"""
    rep = od.open_report(tmpdir, fastq, reg, min_id, min_cov)
    rep.skip_otu()
    for key, ix in reg.items():
        p = smr.default_params()
        p.index_num, p.part = key
        data, groups, any_ = e.otu_part_mates(1, 0, p, ix, min_id, min_cov)
        od.check_groups(data, groups)
        if results is not None:
            results[key] = (data, groups, any_)
        rep.add_otu(key[0], key[1], data, groups, any_)
    feed_pairs(rep, reads, recs)
    rep.close()
    return od.map_file(tmpdir), rep.total_otu


def ids_of(data, groups):
    """-> per group, the list of its ids"""
    ends = [int(g["off"]) for g in groups[1:]] + [len(data)]
    return [data[int(g["off"]):end].split(b"\t") for g, end in zip(groups, ends)]


# ------------------------------------------------------------------------------------------------ 1. crafted state
def crafted_body(engine, n, shape, fastq, tmp_path, long_at=None):
    A, B, members = craft_pairs(n, shape, fastq, seed=n + 1, long_at=long_at)
    pr = Pair(engine, A, B)
    e = pr.e
    try:
        pr.run_pass()
        recs = pr.records()
        what = "%d pairs, %s, fastq=%s" % (n, shape, fastq)
        host = host_map(tmp_path / "host", pr.reads, recs, fastq, pr.reg)
        res = {}
        dev = device_map(tmp_path / "dev", e, pr.reads, recs, fastq, pr.reg, results=res)
        assert dev[0] == host[0], "%s: otu_map.txt differs" % what
        assert dev[1] == host[1], "%s: the number of groups differs" % what
        assert host[0] is not None and host[0].count(b"\n") == host[1]
        got = sum(int(g["n_reads"]) for key in res for g in res[key][1])
        assert got == members, "%s: crafted for %d members, the device found %d" % (what, members, got)
        assert all(r[2] for r in res.values())
        ids = [x for key in res for grp in ids_of(*res[key][:2]) for x in grp]
        id_a = {pr.reads[0].record_text(i)[0].split(" ")[0].lstrip(">@").encode() for i in range(n)}
        id_b = {pr.reads[1].record_text(i)[0].split(" ")[0].lstrip(">@").encode() for i in range(n)}
        assert not (id_a & id_b) and set(ids) <= (id_a | id_b)
        from_a, from_b = sum(x in id_a for x in ids), sum(x in id_b for x in ids)
        if shape == "a only":
            assert from_a == members and from_b == 0
        elif shape == "b only":
            assert from_b == members and from_a == 0
        elif shape == "one":
            grp = res[(0, 0)][1]
            assert len(grp) == 1 and int(grp[0]["n_reads"]) == 4 * n and res[(1, 0)][1].shape[0] == 0      # 1025 pairs: more than 1024 members in one group
            assert ids == [x for i in range(n) for x in 2 * [pr.reads[0].record_text(i)[0].split(" ")[0].lstrip(">@").encode()] +
                           2 * [pr.reads[1].record_text(i)[0].split(" ")[0].lstrip(">@").encode()]]      # pair order, mate 1 before mate 2, then slot order
        elif n >= 63:
            assert set(A.kinds) == set(KINDS), set(KINDS) - set(A.kinds)
            assert from_a > 0 and from_b > 0
            assert any(int(g["n_reads"]) > 1 and {x in id_a for x in grp} == {True, False}
                       for key in res for g, grp in zip(res[key][1], ids_of(*res[key][:2]))), "no group holds members of both batches"
        if long_at is not None:
            assert any(len(x) > 4096 for x in ids) and any(len(x) <= 4 for x in ids)
            big = [grp for key in res for grp in ids_of(*res[key][:2]) if any(len(x) > 4096 for x in grp)]
            assert all(len(grp) > 1 for grp in big) and all(x in id_b for grp in big for x in grp if len(x) > 4096)      # in a group with short ids around it; batch B's
        p = smr.default_params()                                     # (key (0, 0) holds members in every shape: the times of a call that went all the way)
        assert e.otu_part_mates(1, 0, p, pr.ix, MIN_ID, MIN_COV)[0] == res[(0, 0)][0] != b""
        t, tm = e.otu_times(), e.otu_mates_times()
        assert tm["classify_a"] > 0 and tm["sizes_a"] > 0 and tm["classify_b"] > 0 and tm["sizes_b"] > 0 and tm["compact"] > 0, tm
        assert t["classify"] > 0 and t["sort"] >= 0 and t["write"] > 0, t
        assert pr.records() == recs                                  # no stored state changed, and batch 0 is selected again
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ 2. the reference's paired fixture in two batches
def paired_body(engine, case, tmp_path):
    """paired_1.fastq in the selected batch, paired_2.fastq in batch 1; the reference's records after the pass are imported mate by mate with the
    counters taken out, the pass puts them back on both batches.  Every file of the device report equals the host writer's; the ids in each
    aligned_denovo.* file equal the fixture's; for the cases with a map of the reference's (paired_loose, paired_loose_in), that file is this
    map's lines without the ids of second mates -- byte equality is not to be had, see below.  -> does the case have such a map"""
    from . import paths, refrun
    g = otu.load()[case]
    want = otu.records(case)
    paired = os.path.join(paths.GOLDEN, "paired")
    opt = dict(paired_in="-paired_in" in g["options"], out2="-out2" in g["options"], sout="-sout" in g["options"])
    parts = smr.Index.build(os.path.join(paths.GOLDEN, "real_db.fasta"), 18, 3072.0, 10000, 0)
    reg = {(0, j): ix for j, ix in enumerate(parts)}
    slots = max([len(refrun.parse_record(r)["alignv"]) for r in want if r] + [1])
    e = engine()
    reads = []
    try:
        for j, ix in enumerate(parts):
            e.upload_index(ix, j)
        for k in (0, 1):
            e.select_batch(k)
            reads.append(e.upload_fastx(open(os.path.join(paired, "paired_%d.fastq" % (k + 1)), "rb").read(), slots, view=True, keep=True))
            mine = want[k::2]
            assert reads[k].count == len(mine)
            e.import_state([r[:8] + bytes(16) + r[24:] if r else r for r in mine])
            od.run_pass(e, reg, lambda key: smr.default_params(), g["min_id"], g["min_cov"], slot_of=lambda key: key[1])
            assert e.export_records() == mine
        e.select_batch(0)
        recs = [want[0::2], want[1::2]]
        m1, m2 = ([r.record_text(i) for i in range(r.count)] for r in reads)
        host = od.open_report(tmp_path / "host", True, reg, g["min_id"], g["min_cov"], **opt)
        dev = od.open_report(tmp_path / "dev", True, reg, g["min_id"], g["min_cov"], **opt)
        dev.skip_otu()
        dev.skip_denovo()
        feed_pairs(host, reads, recs)
        feed_pairs(dev, reads, recs)
        for key, ix in reg.items():
            p = smr.default_params()
            p.index_num, p.part = key
            d, groups, any_ = e.otu_part_mates(1, key[1], p, ix, g["min_id"], g["min_cov"])
            od.check_groups(d, groups)
            dev.add_otu(key[0], key[1], d, groups, any_)
        dev.add_denovo(e.fastx_denovo(layout=2, mates=1, **opt))
        host.close()
        dev.close()
        for k in (0, 1):
            e.select_batch(k)
            assert e.export_records() == recs[k]
    finally:
        e.close()
        for r in reads:
            r.free()
        for ix in parts:
            ix.free()
    names = sorted(os.listdir(str(tmp_path / "host")))
    assert names == sorted(os.listdir(str(tmp_path / "dev"))) and ("otu_map.txt" in names) == g["otu_map_exists"]
    for fn in names:
        assert open(tmp_path / "dev" / fn, "rb").read() == open(tmp_path / "host" / fn, "rb").read(), "%s: %s differs from the host writer's" % (case, fn)
    got = {fn: [l.split()[0][1:] for l in open(tmp_path / "dev" / fn).readlines()[0::4]] for fn in names if fn.startswith("aligned_denovo")}
    assert got == g["denovo_files"]
    assert dev.total_otu == host.total_otu
    ref_map = os.path.join(otu.OTU_DIR, case + ".otu_map.txt")
    assert os.path.isfile(ref_map) == g["otu_map_exists"]
    if g["otu_map_exists"]:
        # The reference's own file.  With two mate files its fill_otu_map2 reads the first mate file alone at -threads 1 (otumap.cpp:144): mates
        # of the second file never reach its map (here the file is EMPTY: the one read that passed is a second mate).  That quirk depends on the
        # thread count and is not reproduced by the host writer (test_otu_cpu.py pins this); so the file cannot be equal byte for byte, and
        # is compared as that test compares it: the reference's lines are this map's lines with the ids of second mates taken out
        import struct
        ours = [l.rstrip("\n").split("\t") for l in open(tmp_path / "dev" / "otu_map.txt")]
        ref_lines = [l.rstrip("\n").split("\t") for l in open(ref_map)]
        first_ids = {m1[i][0].split()[0].lstrip("@") for i in range(len(recs[0]))}
        second_only = {m2[i][0].split()[0].lstrip("@") for i in range(len(recs[1]))} - first_ids
        passed = [(k, struct.unpack_from("<4I", r, 8)[0]) for k in (0, 1) for r in recs[k] if r and struct.unpack_from("<4I", r, 8)[0] > 0]
        assert passed and sum(len(l) - 1 for l in ours) == sum(n for _, n in passed) and dev.total_otu == len(ours) > 0
        if not second_only:                 # (mates share their id in these files: the first-mate lines cannot be told apart by id)
            assert all(k == 1 for k, _ in passed) and ref_lines == []
        else:
            assert [[l[0]] + [x for x in l[1:] if x not in second_only] for l in ours if any(x not in second_only for x in l[1:])] == ref_lines
    return g["otu_map_exists"]


# ------------------------------------------------------------------------------------------------ 3. contract and refusals
def call(e, mates, slot, p, ix, min_id, min_cov, buf, cap, groups, gcap):
    need = (C.c_uint64 * 2)(9, 9)
    any_ = C.c_int(9)
    rc = e.L.smr_otu_part_mates(e.h, mates, slot, C.byref(p) if p is not None else None, ix.h if ix is not None else None, min_id, min_cov,
                                buf.ctypes.data if buf is not None else None, cap, groups.ctypes.data if groups is not None else None, gcap, need, C.byref(any_))
    return rc, list(need), any_.value


def contract_body(engine, tmp_path):
    ix, refs = od.crafted_db()
    A, B, members = craft_pairs(130, "mixed", True, seed=9)
    pr = Pair(engine, A, B)
    e, reads = pr.e, pr.reads
    p = smr.default_params()
    G = smr.engine.OTU_GROUP
    thr = (MIN_ID, MIN_COV)
    try:
        # two batches on which the pass never ran: no error, nothing
        assert call(e, 1, 0, p, ix, *thr, None, 0, None, 0) == (0, [0, 0], 0)
        # the pass on batch B only, on batch A only: the members of that batch, as many as the host writer finds
        base = pr.records()
        for only in (1, 0):
            pr.run_pass(batches=(only,))
            recs1 = pr.records()
            host1 = host_map(tmp_path / ("host_only%d" % only), reads, recs1, True, pr.reg)
            dev1 = device_map(tmp_path / ("dev_only%d" % only), e, reads, recs1, True, pr.reg)
            assert dev1 == host1 and host1[1] > 0, only
            e.select_batch(only)
            e.reset_state()
            e.import_state(base[only])
            e.select_batch(0)
        assert call(e, 1, 0, p, ix, *thr, None, 0, None, 0) == (0, [0, 0], 0)
        pr.run_pass()
        recs = pr.records()
        plain0 = e.otu_part(0, p, ix, *thr)                          # the selected batch's own map, before

        def still_fine():
            got = e.otu_part(0, p, ix, *thr)
            assert got[0] == plain0[0] and got[1].tobytes() == plain0[1].tobytes() and got[2] == plain0[2]      # batch 0 is still the selected one

        # sizes only
        rc, need, any_ = call(e, 1, 0, p, ix, *thr, None, 0, None, 0)
        assert rc == 0 and need[0] > 0 and need[1] > 0 and any_ == 1
        t = e.otu_times()
        assert t["write"] == 0 and t["d2h"] == 0 and t["classify"] > 0, t
        buf = np.full(need[0] + 64, 0x5A, dtype=np.uint8)
        grp = np.zeros(need[1] + 4, dtype=G)
        grp.view(np.uint8)[:] = 0x5A
        full = (buf, len(buf), grp, len(grp))

        def refused(got, want, *words):
            msg = e.L.smr_last_error(e.h).decode()
            assert got == want and "smr_otu_part_mates" in msg and all(w in msg for w in words), (got, want, words, msg)
            assert (buf == 0x5A).all() and (grp.view(np.uint8) == 0x5A).all()
            still_fine()

        # one short in either: refused, nothing written, the sizes valid
        for cap, gcap in ((need[0] - 1, need[1]), (need[0], need[1] - 1)):
            rc, need2, _ = call(e, 1, 0, p, ix, *thr, buf, cap, grp, gcap)
            assert need2 == need
            refused(rc, ERR_CAPACITY)
        # exactly the sizes: nothing behind them
        rc, need2, _ = call(e, 1, 0, p, ix, *thr, buf, need[0], grp, need[1])
        assert rc == 0 and need2 == need and (buf[need[0]:] == 0x5A).all() and (grp[need[1]:].view(np.uint8) == 0x5A).all()
        first, first_g = buf[:need[0]].tobytes(), grp[:need[1]].tobytes()
        od.check_groups(first, grp[:need[1]])
        still_fine()
        # again: the same
        buf[:] = 0x5A
        grp.view(np.uint8)[:] = 0x5A
        assert call(e, 1, 0, p, ix, *thr, *full)[0] == 0
        assert buf[:need[0]].tobytes() == first and grp[:need[1]].tobytes() == first_g and (buf[need[0]:] == 0x5A).all()
        buf[:] = 0x5A
        grp.view(np.uint8)[:] = 0x5A

        def good():
            assert call(e, 1, 0, p, ix, *thr, *full)[0] == 0 and buf[:need[0]].tobytes() == first and grp[:need[1]].tobytes() == first_g
            buf[:] = 0x5A
            grp.view(np.uint8)[:] = 0x5A

        # 1. the call's own arguments
        refused(call(e, 1, 0, p, None, *thr, *full)[0], ERR_ARG)
        refused(call(e, 1, 0, None, ix, *thr, *full)[0], ERR_ARG)
        refused(call(e, 1, 64, p, ix, *thr, *full)[0], ERR_ARG, "slot")
        refused(call(e, 1, -1, p, ix, *thr, *full)[0], ERR_ARG, "slot")
        for m in (-1, 16, 0):
            refused(call(e, m, 0, p, ix, *thr, *full)[0], ERR_ARG, "mates")
        for bad in ((1.5, 0.5), (0.5, -0.1), (float("nan"), 0.5)):
            refused(call(e, 1, 0, p, ix, *bad, *full)[0], ERR_ARG, "min_id")
            refused(call(e, 2, 5, p, ix, *bad, *full)[0], ERR_ARG, "min_id")           # before the state of the slot and of batch 2
        refused(call(e, 16, 5, p, ix, *thr, *full)[0], ERR_ARG, "mates")                # before the plain call's refusals
        good()
        # 2. the plain call's refusals for the selected batch, each before anything of batch `mates` (batch 2 holds nothing)
        refused(call(e, 2, 5, p, ix, *thr, *full)[0], ERR_STATE, "slot empty")
        other = smr.Index.build(golden.inputs("t9")[0], 18, 3072.0, 10000, 0)[0]
        refused(call(e, 2, 0, p, other, *thr, *full)[0], ERR_ARG, "resident")
        other.free()
        s = refs[20][:100]
        ok, cold = od.m_aln(20, 0, 100, 0, 100), od.m_aln(21, 0, 100, 0, 100)
        bad_sets = {"a CIGAR past its read": (dict(ok, cigar=[(101 << 4) | 0]), ERR_ARG),
                    "a CIGAR past its reference": (dict(ok, ref_begin1=len(refs[20]) - 99), ERR_ARG),
                    "a negative start": (dict(ok, read_begin1=-1), ERR_ARG),
                    "ref_num beyond the part": (dict(ok, ref_num=od.N_REFS), ERR_ARG),
                    "no CIGAR": (dict(ok, cigar=[]), ERR_STATE)}
        # batches 3 and 4: two reads each; the bad alignment belongs to key (1, 0), on which the pass is not run (it would walk it); the read's
        # good alignment of key (0, 0) puts its c_yid_ycov above 0.  In a read whose counter is 0 (`cold`) the same alignment is not looked at
        G2 = od.Batch(True, slots=2)
        G2.add("guard", s, [])
        G2.add("cold", "ACGT" * 25, [])
        p1 = smr.default_params()
        p1.index_num = 1
        small = []
        for k in (3, 4):
            e.select_batch(k)
            small.append(e.upload_fastx(G2.text(), G2.slots, view=True, keep=True))
        clean = [rows.record([ok], 2), rows.record([cold], 2)]

        def load(k, recs_k):
            e.select_batch(k)
            e.reset_state()
            e.import_state(recs_k)
            od.run_pass(e, {(0, 0): ix}, lambda key: smr.default_params(), *thr)
            assert e.idcov_counters()["n_yid_ycov"] == 1
            e.select_batch(3)

        for what, (aln, want_rc) in bad_sets.items():
            bad = dict(aln, index_num=1)
            dirty = [rows.record([ok, bad], 2), rows.record([cold, bad], 2)]
            # in the selected batch (3): refused before batch `mates` is looked at -- batch 2 holds nothing, and the message names no batch
            load(4, clean)
            load(3, dirty)
            for mates in (2, 4):
                rc = call(e, mates, 0, p1, ix, *thr, *full)[0]
                msg = e.L.smr_last_error(e.h).decode()
                assert rc == want_rc and "smr_otu_part_mates" in msg and "batch" not in msg, (what, mates, rc, msg)
                assert (buf == 0x5A).all() and (grp.view(np.uint8) == 0x5A).all(), what
            # 5. in batch `mates` (4): the message names the batch
            load(3, clean)
            load(4, dirty)
            rc = call(e, 4, 0, p1, ix, *thr, *full)[0]
            msg = e.L.smr_last_error(e.h).decode()
            assert rc == want_rc and "smr_otu_part_mates" in msg and "batch 4" in msg, (what, rc, msg)
            assert (buf == 0x5A).all() and (grp.view(np.uint8) == 0x5A).all(), what
            # only in reads whose counter is 0: not looked at
            load(4, [rows.record([ok], 2), rows.record([cold, bad], 2)])
            rc, need3, any3 = call(e, 4, 0, p1, ix, *thr, *full)
            assert (rc, need3, any3) == (0, [0, 0], 1), (what, rc, need3, any3)
            # after a refusal a good call succeeds
            rc, need3, any3 = call(e, 4, 0, p, ix, *thr, *full)
            assert rc == 0 and need3 == [len(b"guard\tguard"), 1] and buf[:need3[0]].tobytes() == b"guard\tguard", (what, rc, need3)
            buf[:] = 0x5A
            grp.view(np.uint8)[:] = 0x5A
        for r in small:
            r.free()
        e.select_batch(0)
        good()
        # a selected batch without kept text
        plain = smr.Reads.from_seqs([reads[0].record_text(i)[1] for i in range(reads[0].count)])
        e.select_batch(5)
        e.upload_reads(plain, A.slots)
        e.import_state(A.records())
        assert call(e, 2, 0, p, ix, *thr, *full)[0] == ERR_STATE and "SMR_FASTX_KEEP" in e.L.smr_last_error(e.h).decode() and "batch 2" not in e.L.smr_last_error(e.h).decode()
        e.select_batch(0)
        # 3. batch `mates` without reads, or without their text (before its unequal count)
        refused(call(e, 2, 0, p, ix, *thr, *full)[0], ERR_STATE, "SMR_FASTX_KEEP", "batch 2")
        refused(call(e, 5, 0, p, ix, *thr, *full)[0], ERR_STATE, "SMR_FASTX_KEEP", "batch 5")
        plain.free()
        plain = smr.Reads.from_seqs([reads[0].record_text(i)[1] for i in range(5)])
        e.select_batch(5)
        e.upload_reads(plain, A.slots)
        e.select_batch(0)
        plain.free()
        refused(call(e, 5, 0, p, ix, *thr, *full)[0], ERR_STATE, "SMR_FASTX_KEEP", "batch 5")
        # 4. unequal read counts; FASTA against FASTQ
        A5, _, _ = craft_pairs(5, "mixed", True, seed=3)
        e.select_batch(6)
        r5 = e.upload_fastx(A5.text(), A5.slots, view=True, keep=True)
        e.select_batch(0)
        refused(call(e, 6, 0, p, ix, *thr, *full)[0], ERR_ARG, "130 reads, 5 mates")
        r5.free()
        Aa, _, _ = craft_pairs(130, "mixed", False, seed=4)
        e.select_batch(6)
        ra = e.upload_fastx(Aa.text(), Aa.slots, view=True, keep=True)
        e.import_state(Aa.records())
        e.select_batch(0)
        refused(call(e, 6, 0, p, ix, *thr, *full)[0], ERR_ARG, "FASTA reads with FASTQ mates")
        ra.free()
        good()
        # two empty batches
        e.select_batch(7)
        e.upload_fastx(b"", 2, view=True, keep=True).free()
        e.select_batch(8)
        e.upload_fastx(b"", 2, view=True, keep=True).free()
        assert call(e, 7, 0, p, ix, *thr, *full) == (0, [0, 0], 0)
        assert (buf == 0x5A).all() and (grp.view(np.uint8) == 0x5A).all()
        e.select_batch(0)
        # the context goes on working: the same bytes, and no stored state has changed
        good()
        still_fine()
        assert pr.records() == recs
    finally:
        pr.close()
