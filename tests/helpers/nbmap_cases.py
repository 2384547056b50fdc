"""Bodies of the search-bitmap tests (csrc/smr_nbmap.hpp), shared by tests/test_gpu_nbmap.py (-m gpu) and tests/test_emu_nbmap.py (the same kernel
source on the emulator).  Every body creates its own engine: a context latches the switches when it is created."""
import bisect

import numpy as np

import sortmerna_amd as smr
from sortmerna_amd import synth

from . import nbmap

GIB = 1 << 30


def expected_drop(nk, pw, drop, budget):
    """the policy of build_nbmap (smr_engine.hip): chars left out so that a slab fits 32 KB and the map its budget; None: no bitmap"""
    while drop < pw and pw - drop >= 4 and (pw - drop > 9 or 2 * nk * nbmap.slab_words(pw, drop) * 4 > budget):
        drop += 1
    return None if drop >= pw or pw - drop < 4 else drop


def force(monkeypatch, drop, budget=None, **env):
    monkeypatch.setenv("SMR_SEED_NBMAP", "2")
    monkeypatch.setenv("SMR_SEED_NBMAP_DROP", str(drop))
    if budget is not None:
        monkeypatch.setenv("SMR_SEED_NBMAP_BYTES", str(budget))
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _sample_blocks(root3, limit):
    """block table entries worth comparing: the largest, blocks with and without directories, absent ones, both directions"""
    r3 = np.asarray(root3, dtype=np.uint32).reshape(-1, 2)
    nb = len(r3)
    if nb <= limit:
        return list(range(nb))
    present = r3[:, 0] != nbmap.NONE
    n, cA = r3[:, 1] & 0xFFFFFF, (r3[:, 1] >> 24) & 15
    pick = []
    for d in (0, 1):
        side = np.arange(nb) % 2 == d
        big = np.nonzero(present & side)[0]
        pick += list(big[np.argsort(n[big])[-6:]])                                   # the largest
        pick += list(np.nonzero(present & side & (cA > 0))[0][:6])                   # with directories
        pick += list(np.nonzero(present & side & (cA == 0))[0][:6])                  # without
        pick += list(np.nonzero(~present & side)[0][:3])                             # no mini-trie: a zero slab
    pick += [0, 1, nb - 2, nb - 1]
    return sorted(set(int(x) for x in pick))


def builder_body(tmp_path, monkeypatch, lnwin, db_nt, drop, host_layout, budget=None):
    """the slabs the device builds == a host computation from the part's pigeonhole layout (every pattern against every string of the block where
    that is affordable, the verified candidate list otherwise); the map has the size the policy gives it"""
    force(monkeypatch, drop, budget, **({"SMR_PG_HOST": "1"} if host_layout else {}))
    pw = lnwin // 2
    db = str(tmp_path / "db.fasta")
    synth.make_db(db, db_nt, seed=11, family_size=25)
    part = smr.Index.build(db, lnwin, 3072.0, 10000, 0)[0]
    e = smr.Engine(0)
    try:
        e.upload_index(part, 0)
        info = e.seed_nbmap_info(0)
        pg, root3 = smr.pigeonhole_layout(part)
        nk = len(root3) // 4
        eff = expected_drop(nk, pw, drop, budget if budget is not None else 24 * GIB)
        assert eff is not None and info["built"] == 1 and info["drop"] == eff, (info, eff)
        words = nbmap.slab_words(pw, eff)
        assert info["bytes"] == 2 * nk * words * 4
        r3 = np.asarray(root3, dtype=np.uint32).reshape(-1, 2)
        present = r3[:, 0] != nbmap.NONE
        assert info["tries"] == int(present.sum()) and info["strings"] == int((r3[present, 1] & 0xFFFFFF).sum())
        blocks = _sample_blocks(root3, 2048 if pw <= 5 else 0)
        shapes = set()
        for i in blocks:
            got = e.seed_nbmap_fetch(0, i, 1, words)
            n = int(r3[i, 1] & 0xFFFFFF) if present[i] else 0
            brute = n * (1 << (2 * pw)) <= (1 << 23)
            exp = nbmap.host_slabs(pg, root3, pw, eff, [i], brute=brute)
            assert np.array_equal(got, exp), "block %d (%d strings, %s): %d words differ" % (i, n, "brute" if brute else "candidates", int((got != exp).sum()))
            if present[i]:
                assert got.any()
                shapes.add(bool((int(r3[i, 1]) >> 24) & 15))
            else:
                assert not got.any()
        assert shapes == {True, False} or (pw <= 5 and shapes), shapes       # blocks with and without directories (an L = 10 part of this size has only the former)
        assert set(b & 1 for b in blocks if present[b]) == {0, 1}            # both directions
    finally:
        e.close()


def _scan_all(e, wl):
    """{(strand, pass): (number of hits, sorted (read, id, window) triples)} of smr_seed_scan over the workload"""
    e.upload_reads(wl.reads, 1)
    e.upload_index(wl.parts[0], 0)
    p = smr.default_params(minimal_score=wl.minimal_score)
    out = {}
    for strand in (0, 1):
        for pass_ in (0, 1, 2):
            e.reset_state()
            n = e.seed_scan(0, p, strand, pass_)
            got = e.seed_hits()
            out[(strand, pass_)] = (n, np.array(sorted(map(tuple, got.tolist())), dtype=np.int64).reshape(-1, 3))
    return out


def census(e, before=None):
    i = e.seed_nbmap_info(0)
    c = {k: i[k] for k in ("probed", "passed", "empty")}
    if before:
        c = {k: c[k] - before[k] for k in c}
    return c


def assert_filtered(c, what=""):
    """the launches really took the filtered path: searches were probed, some passed, most did not, and some of the passed accepted a string"""
    assert c["probed"] > c["passed"] > c["empty"] >= 0 and c["probed"] - c["passed"] > 100, (what, c)


def scan_parity_body(wl, monkeypatch, drop, budget=None):
    """hit counts and window segments of every (strand, pass) with the filter forced == without a bitmap"""
    monkeypatch.setenv("SMR_SEED_NBMAP", "0")
    e = smr.Engine(0)
    try:
        plain = _scan_all(e, wl)
        assert not e.seed_nbmap_info(0)["built"] and census(e)["probed"] == 0
    finally:
        e.close()
    force(monkeypatch, drop, budget)
    e = smr.Engine(0)
    try:
        filt = _scan_all(e, wl)
        info = e.seed_nbmap_info(0)
        assert info["built"] == 1
        assert_filtered(census(e), "seed_scan drop %d" % info["drop"])
    finally:
        e.close()
    for k in plain:
        assert plain[k][0] == filt[k][0] > 0, (k, plain[k][0], filt[k][0])
        # the same (read, id, window) triples: a search the filter left out had no hit in the unfiltered run (which
        # test_seed_scan_matches_oracle ties to the oracle's traversal)
        assert np.array_equal(plain[k][1], filt[k][1]), k
    return info


def records_parity_body(wl, monkeypatch, drop, budget=None, env=None, **opts):
    """smr_align_part's records with the filter forced == the oracle's"""
    force(monkeypatch, drop, budget, **(env or {}))
    recs_o, ctr_o = wl.oracle_records(**opts)
    e = smr.Engine(0)
    try:
        recs_g, ctr_g = wl.gpu_records(e, **opts)
        assert_filtered(census(e), "align drop %d %s" % (drop, env))          # (smr.align has unloaded the part: the batch's counters say what ran)
    finally:
        e.close()
    bad = [i for i, (a, b) in enumerate(zip(recs_g, recs_o)) if a != b]
    assert len(recs_g) == len(recs_o) and not bad, "%d of %d records differ from the oracle's (first: read %d)" % (len(bad), len(recs_o), bad[0])
    assert ctr_g["num_aligned"] == ctr_o["num_aligned"] > 100 and ctr_g["num_short"] == ctr_o["num_short"]
    assert ctr_g["reads_matched_per_db"][0] == ctr_o["per_db"]


def _pg_key(T, frm, cnt):
    k = 0
    for q in range(cnt):
        k = (k << 2) | ((T >> (2 * (frm + q))) & 3)
    return k


def filtered_search_bytes(pg, root3, tuples, cbase, meta, direction, zero_slots, pw, drop):
    """What the filter changes in k_seed_pg<direction>'s byte count against the unfiltered recount (test_gpu_parity._host_recount_of_the_search):
    + 4 B per tuple decoded (its bitmap word; a repeated seed is not decoded), and for every search whose bit is clear -- no string of its block
    accepts any pattern with the same first pw - drop chars -- none of its directory words (32 B) and none of the strings of its ranges (4 B each).
    -> (difference in bytes, searches probed, searches passed)"""
    h = pw // 2
    n_fwd, n_all, fb, cb, nkh = meta["n_fwd"], meta["n"], meta["fb"], meta["cb"], meta["nkh"]
    lo, hi = (0, n_fwd) if direction == 0 else (n_fwd, n_all)
    cb_list = [int(x) for x in cbase]
    keep = (1 << (2 * (pw - drop))) - 1
    tails = (np.arange(1 << (2 * drop), dtype=np.uint64) << np.uint64(2 * (pw - drop)))
    delta = probed = passed = 0
    for i in range(lo, hi):
        t = int(tuples[i])
        if t >> 63:
            continue
        delta += 4
        slot, P = t & 0xFFFFFFFF, (t >> 32) & ((1 << cb) - 1)
        if direction == 1 and slot in zero_slots:
            continue
        probed += 1
        c = bisect.bisect_right(cb_list, i) - 1
        key = (c << fb) | (t >> (32 + cb))
        e = 2 * (2 * (key - (nkh if direction else 0)) + direction)
        off4, metaw = int(root3[e]), int(root3[e + 1])
        if off4 == 0xFFFFFFFF:
            continue                                               # (a zero slab; the unfiltered search read nothing either)
        T = nbmap.strings_of_block(pg, off4, metaw).astype(np.uint64)
        if nbmap.accepts((np.uint64(P & keep) | tails)[None, :], T[:, None], pw).any():
            passed += 1
            continue
        n, cA, cB = metaw & 0xFFFFFF, (metaw >> 24) & 15, metaw >> 28
        if cA == 0:
            delta -= 4 * n
            continue
        blk = off4 * 4
        nA = (1 << (2 * cA)) + 1
        dirA, dirB = blk, blk + nA
        kA, kb0, kb1 = _pg_key(P, 0, cA), _pg_key(P, h, cB), _pg_key(P, h - 1, cB)
        if cB == pw - h:
            lo2 = 4 * _pg_key(P, h + 1, cB - 1); hi2 = lo2 + 4
        else:
            lo2 = _pg_key(P, h + 1, cB); hi2 = lo2 + 1
        cnt = int(pg[dirA + kA + 1]) - int(pg[dirA + kA]) + int(pg[dirB + kb0 + 1]) - int(pg[dirB + kb0]) + int(pg[dirB + hi2]) - int(pg[dirB + lo2])
        if kb1 != kb0:
            cnt += int(pg[dirB + kb1 + 1]) - int(pg[dirB + kb1])
        delta -= 32 + 4 * cnt
    return delta, probed, passed


def two_refs_body(tmp_path, monkeypatch, drop, budget=None):
    """two --ref, the first cut into several index parts (every part gets a bitmap of its own): records == the oracle's"""
    import os
    from . import orc
    from .workload import Workload
    force(monkeypatch, drop, budget)
    os.makedirs(str(tmp_path / "a"))
    w1 = Workload(str(tmp_path / "a"), db_nt=260_000, n_reads=1800, seed=91, frac_db=0.5, n_rate=0.004, max_mb=0.5)
    assert w1.stats.nparts >= 3
    os.makedirs(str(tmp_path / "b"))
    out, keep, k = [], True, 0                               # the second DB: a third of the first one's sequences, every 50th letter changed
    for line in open(w1.db):
        if line.startswith(">"):
            k += 1
            keep = k % 3 == 0
            if keep:
                out.append(line)
        elif keep:
            a = list(line.rstrip("\n"))
            for i in range(7, len(a), 50):
                a[i] = "ACGT"[("ACGT".index(a[i]) + 1) & 3] if a[i] in "ACGT" else a[i]
            out.append("".join(a) + "\n")
    db2 = str(tmp_path / "b" / "second.fasta")
    open(db2, "w").write("".join(out))
    w2 = Workload(str(tmp_path / "b"), db_fasta=db2, seqs=w1.seqs)
    ws = [w1, w2]
    run = orc.Run(w1.seqs)
    for k, x in enumerate(ws):
        for part in range(x.stats.nparts):
            po = orc.default_params(minimal_score=x.minimal_score, num_alignments=2)
            po.index_num, po.part, po.is_last_index_part = k, part, int(k == 1 and part == x.stats.nparts - 1)
            run.align_part(x.prefix, x.db, x.stats, part, po)
    recs_o = run.records()
    n_al = run.counters.num_aligned
    run.close()
    e = smr.Engine(0)
    try:
        ps = [smr.default_params(minimal_score=x.minimal_score, num_alignments=2) for x in ws]
        smr.align(e, w1.reads, [x.parts for x in ws], ps)
        recs_g = e.records()
        assert e.counters(2)["num_aligned"] == n_al > 300
        assert_filtered(census(e), "two references")
    finally:
        e.close()
    bad = [i for i, (a, b) in enumerate(zip(recs_g, recs_o)) if a != b]
    assert len(recs_g) == len(recs_o) and not bad, "%d of %d records differ from the oracle's (first: read %d)" % (len(bad), len(recs_o), bad[0])


def _info_after_upload(part):
    e = smr.Engine(0)
    try:
        e.upload_index(part, 0)
        return e.seed_nbmap_info(0)
    finally:
        e.close()


def policy_body(wl, tmp_path, monkeypatch):
    """mode 1 (the default) builds nothing on a sparse part, a map of the expected size once the density threshold is lowered, a smaller one under
    a byte budget, none when nothing of four chars fits; a part whose map finds no memory is searched unfiltered, without an error"""
    for name in ("SMR_SEED_NBMAP", "SMR_SEED_NBMAP_DROP", "SMR_SEED_NBMAP_MIN", "SMR_SEED_NBMAP_BYTES", "SMR_SEED_NBMAP_ALLOC_MAX"):
        monkeypatch.delenv(name, raising=False)
    db = str(tmp_path / "db10.fasta")
    synth.make_db(db, 60_000, seed=11, family_size=25)
    small = smr.Index.build(db, 10, 3072.0, 10000, 0)[0]            # pw = 5: 2048 slabs of 128 bytes at the exact set
    full = 2 * 1024 * 128
    for part in (wl.parts[0], small):
        i = _info_after_upload(part)
        assert i["built"] == 0 and i["bytes"] == 0 and 0 < i["strings"] < 128 * i["tries"], i      # the default: too sparse to pay
    monkeypatch.setenv("SMR_SEED_NBMAP_MIN", "1")
    i = _info_after_upload(small)
    assert (i["built"], i["drop"], i["bytes"]) == (1, 1, full // 4), i      # the default leaves one char out
    monkeypatch.setenv("SMR_SEED_NBMAP_DROP", "0")
    i = _info_after_upload(small)
    assert (i["built"], i["drop"], i["bytes"]) == (1, 0, full), i
    monkeypatch.setenv("SMR_SEED_NBMAP_BYTES", str(full // 2))
    i = _info_after_upload(small)
    assert (i["built"], i["drop"], i["bytes"]) == (1, 1, full // 4), i      # the budget raises the drop
    monkeypatch.setenv("SMR_SEED_NBMAP_BYTES", str(full // 8))
    i = _info_after_upload(small)
    assert i["built"] == 0 and i["bytes"] == 0, i                           # pw - drop < 4: none
    monkeypatch.delenv("SMR_SEED_NBMAP_BYTES")
    monkeypatch.setenv("SMR_SEED_NBMAP", "0")
    assert _info_after_upload(small)["built"] == 0
    # no room for the map: the part goes without a filter and aligns as ever
    monkeypatch.setenv("SMR_SEED_NBMAP", "2")
    monkeypatch.setenv("SMR_SEED_NBMAP_DROP", "4")
    monkeypatch.setenv("SMR_SEED_NBMAP_ALLOC_MAX", "1000")
    recs_o, ctr_o = wl.oracle_records()
    e = smr.Engine(0)
    try:
        recs_g, ctr_g = wl.gpu_records(e)
        i = e.seed_nbmap_info(0)
        assert i["built"] == 0 and i["bytes"] == 0 and i["probed"] == 0, i
    finally:
        e.close()
    assert recs_g == recs_o and ctr_g["num_aligned"] == ctr_o["num_aligned"] > 100


def bytes_body(wl, monkeypatch, strand, pass_, drop, budget=None):
    """C_B_PG0 / C_B_PG1 with the filter forced == the unfiltered host recount of tests/test_gpu_parity.py + what the filter changes
    (filtered_search_bytes); the searches the kernel says it probed and passed == the host's"""
    from test_gpu_parity import _host_recount_of_the_search
    force(monkeypatch, drop, budget)
    e = smr.Engine(0)
    try:
        e.upload_reads(wl.reads, 1)
        e.upload_index(wl.parts[0], 0)
        eff = e.seed_nbmap_info(0)["drop"]
        p = smr.default_params(minimal_score=wl.minimal_score)
        pg, root3 = smr.pigeonhole_layout(wl.parts[0])
        e.reset_state()
        e.prof_reset()
        c0 = census(e)
        e.seed_scan(0, p, strand, pass_)
        tuples, cbase, meta = e.seed_tuples()
        assert meta["redo"] == 0 and meta["n"] > 1000 and 0 < meta["n_fwd"] < meta["n"]
        kp = e.prof_kernels()
        c = census(e, c0)
        exp0, zeros = _host_recount_of_the_search(pg, root3, tuples, cbase, meta, 0, set(), 9)
        exp1, _ = _host_recount_of_the_search(pg, root3, tuples, cbase, meta, 1, zeros, 9)
        d0, pr0, pa0 = filtered_search_bytes(pg, root3, tuples, cbase, meta, 0, set(), 9, eff)
        d1, pr1, pa1 = filtered_search_bytes(pg, root3, tuples, cbase, meta, 1, zeros, 9, eff)
        assert d0 < 0 or d1 < 0                                  # (the filter saved strings and directory words)
        assert (c["probed"], c["passed"]) == (pr0 + pr1, pa0 + pa1), (c, pr0, pr1, pa0, pa1)
        assert_filtered(c, "bytes")
        assert int(kp["k_seed_pg<0>"]["bytes"]) == exp0 + d0, (int(kp["k_seed_pg<0>"]["bytes"]), exp0, d0)
        assert int(kp["k_seed_pg<1>"]["bytes"]) == exp1 + d1, (int(kp["k_seed_pg<1>"]["bytes"]), exp1, d1)
    finally:
        e.close()
