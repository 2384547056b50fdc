"""Two batches of mates and the host writer's answer for the tests of smr_rows_part_mates / smr_pairwise_part_mates and their _gz forms
(test_gpu_rows_mates.py / test_emu_rows_mates.py).  TEST INFRASTRUCTURE ONLY.

The yardstick is always smr_report_add_pair (Report.add_pair, pinned to the reference's files by test_reports_cpu.py): mate 1 of pair i is
read i of batch 0, mate 2 read i of batch 1; both go through it into a temporary directory, and what it wrote is compared with the device's
streams for equality.  For the _gz forms the yardstick is zlib and gzip_lines_batch of the plain bytes."""
import ctypes as C
import json
import os
import struct

import numpy as np

import sortmerna_amd as smr
from sortmerna_amd import capi, report

from . import golden, pairwise, paths, refrun, rows, rowsgzdev

ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -4, -5
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1025]
SEEDS = (1, 2)                                   # batch 0, batch 1 (plus the pair count)
PAIRED = os.path.join(paths.GOLDEN, "paired")

_part = {}


def syn_part():
    """a small real index part (tests/golden/syn_db.fasta), built once per process"""
    if "ix" not in _part:
        _part["ix"] = smr.Index.build(rows.SYN_DB, 18, 3072.0, 10000, 0)[0]
        _part["lens"] = rows.ref_lengths()
    return _part["ix"], _part["lens"]


class Pair:
    """an engine with the part in slot 0 and two crafted batches (helpers/rows.py: craft, one seed per batch) in batches 0 and 1, batch 0
    selected; reads[k], recs[k]: the host parser's view and the records of batch k"""

    def __init__(self, engine, n, fastq, seed=0, long_read=False):
        self.ix, lens = syn_part()
        self.n, self.fastq = n, fastq
        self.reg = {key: self.ix for key in rows.KEYS}
        self.e = engine()
        self.e.upload_index(self.ix, 0)
        self.reads, self.recs = [], []
        for k in (0, 1):
            text, recs, slots = rows.craft(n, fastq, lens, seed=100 * seed + SEEDS[k], long_read=long_read and k == 1)
            # (craft leaves every fourth read of either batch without alignments: here read 5 j + 1 of batch 0 and read 5 j + 2 of batch 1 lose
            # their records as well, so that there are pairs with rows of one mate only)
            recs = [b"" if i % 5 == 1 + k and len(r) < 4000 else r for i, r in enumerate(recs)]
            self.e.select_batch(k)
            self.reads.append(self.e.upload_fastx(text, slots, view=True, keep=True))
            assert self.reads[k].count == n
            self.e.import_state(recs)
            self.recs.append(recs)
        self.e.select_batch(0)

    def close(self):
        self.e.close()
        for r in self.reads:
            r.free()


def feed_pairs(rep, reads, recs):
    for i in range(len(recs[0])):
        rep.add_pair(reads[0].record_text(i) + (recs[0][i],), reads[1].record_text(i) + (recs[1][i],))


def host_rows(tmpdir, reads, recs, fastq, cols, reg, dbs=rows.DB):
    """smr_report_add_pair over the pairs -> (aligned.sam, aligned.blast) as bytes"""
    rep = rows.open_report(tmpdir, fastq, cols, reg, dbs)
    feed_pairs(rep, reads, recs)
    rep.close()
    return rows.files(tmpdir, cols)


def host_pairwise(tmpdir, reads, recs, fastq, reg, dbs=rows.DB):
    rep = pairwise.open_report(tmpdir, fastq, reg, dbs)
    feed_pairs(rep, reads, recs)
    rep.close()
    return pairwise.blast_file(tmpdir)


def device_rows(tmpdir, e, fastq, cols, reg, params_of, dbs=rows.DB, slot_of=None, streams=None, sam=True, feed=None):
    """smr_rows_part_mates per (index, part) + smr_report_add_rows, in a report that skips its own rows -> the two files"""
    rep = rows.open_report(tmpdir, fastq, cols, reg, dbs)
    rep.skip_rows()
    for key, ix in reg.items():
        p = params_of(key)
        p.index_num, p.part = key
        lam, K, fr, fq = dbs[key[0]]
        s, b = e.rows_part_mates(1, slot_of(key) if slot_of else 0, p, ix, sam=sam, blast=cols is not None, cols=" ".join(cols or []), lam=lam, K=K, full_ref=fr, full_read=fq)
        if streams is not None:
            streams[key] = (s, b)
        rep.add_rows(key[0], key[1], s, b)
    if feed:                                      # the pairs go through the report as well, which must add no row
        feed_pairs(rep, *feed)
    rep.close()
    return rows.files(tmpdir, cols)


def device_pairwise(tmpdir, e, fastq, reg, params_of, dbs=rows.DB, slot_of=None, streams=None):
    rep = pairwise.open_report(tmpdir, fastq, reg, dbs)
    rep.skip_pairwise()
    for key, ix in reg.items():
        p = params_of(key)
        p.index_num, p.part = key
        lam, K, fr, fq = dbs[key[0]]
        data = e.pairwise_part_mates(1, slot_of(key) if slot_of else 0, p, ix, lam=lam, K=K, full_ref=fr, full_read=fq)
        if streams is not None:
            streams[key] = data
        rep.add_pairwise(key[0], key[1], data)
    rep.close()
    return pairwise.blast_file(tmpdir)


def rows_of(recs, key):
    """alignments of `key` per read: the rows the read has in each stream of that key"""
    return [sum(1 for a in refrun.parse_record(r)["alignv"] if (a["index_num"], a["part"]) == key) if r else 0 for r in recs]


def input_properties(stream, recs, key, want_phases):
    """asserted, not assumed: pairs with rows in batch 0 only, in batch 1 only, in both and in neither; and (want_phases) rows of both
    batches that begin at all four byte phases of the interleaved stream"""
    ca, cb = rows_of(recs[0], key), rows_of(recs[1], key)
    kinds = {(bool(x), bool(y)) for x, y in zip(ca, cb)}
    if len(ca) >= 63:
        assert kinds == {(True, False), (False, True), (True, True), (False, False)}, kinds
    lines = stream.split(b"\n")[:-1]
    assert len(lines) == sum(ca) + sum(cb)
    at, k, seen = 0, 0, ({0: set(), 1: set()})
    for x, y in zip(ca, cb):
        for which, cnt in ((0, x), (1, y)):
            if cnt:
                seen[which].add(at % 4)
            for _ in range(cnt):
                at += len(lines[k]) + 1
                k += 1
    if want_phases:
        assert seen[0] == {0, 1, 2, 3} and seen[1] == {0, 1, 2, 3}, seen


# ------------------------------------------------------------------------------------------------ 1. crafted state
def crafted_body(engine, n, fastq, tmp_path, long_read=False):
    pr = Pair(engine, n, fastq, seed=n, long_read=long_read)
    e = pr.e
    try:
        par = lambda key: smr.default_params()    # noqa: E731
        host = host_rows(tmp_path / "host", pr.reads, pr.recs, fastq, rows.ALL_COLS, pr.reg)
        streams = {}
        both = device_rows(tmp_path / "both", e, fastq, rows.ALL_COLS, pr.reg, par, streams=streams, feed=(pr.reads, pr.recs))
        assert both[0] == host[0], "%d pairs, fastq=%s: aligned.sam differs" % (n, fastq)
        assert both[1] == host[1], "%d pairs, fastq=%s: aligned.blast differs" % (n, fastq)
        assert rows.strip_header(host[0]) == b"".join(streams[k][0] for k in sorted(streams))
        assert host[1] == b"".join(streams[k][1] for k in sorted(streams))
        for key in rows.KEYS:
            want = sum(rows_of(pr.recs[0], key)) + sum(rows_of(pr.recs[1], key))
            assert streams[key][0].count(b"\n") == want and streams[key][1].count(b"\n") == want, key
        for which in (0, 1):
            input_properties(streams[(0, 0)][which], pr.recs, (0, 0), n >= 255)
        # SAM only; BLAST with all optional columns only
        sam_only = device_rows(tmp_path / "sam", e, fastq, None, pr.reg, par)
        assert sam_only[0] == host[0] and sam_only[1] == b""
        for key, ix in pr.reg.items():
            p = smr.default_params()
            p.index_num, p.part = key
            lam, K, fr, fq = rows.DB[key[0]]
            s, b = e.rows_part_mates(1, 0, p, ix, sam=False, blast=True, cols=" ".join(rows.ALL_COLS), lam=lam, K=K, full_ref=fr, full_read=fq)
            assert s == b"" and b == streams[key][1], key
        # the pairwise text
        assert device_pairwise(tmp_path / "pw", e, fastq, pr.reg, par) == host_pairwise(tmp_path / "pwh", pr.reads, pr.recs, fastq, pr.reg)
        if long_read:
            sam = streams[(0, 0)][0].split(b"\n")
            assert len(max(sam, key=len)) > 8192 and min(len(l) for l in streams[(0, 0)][1].split(b"\n")[:-1]) < 100
            assert len(pr.reads[1].record_text(n // 2)[1]) > 5000 > len(pr.reads[0].record_text(n // 2)[1])      # the 5 kb read is batch 1's
        p = smr.default_params()
        p.index_num, p.part = 0, 0
        assert any(e.rows_part_mates(1, 0, p, pr.ix, sam=True, blast=False))
        t = e.mates_times()
        assert t["selected"] > 0 and t["mates"] > 0 and t["interleave"] > 0 and t["d2h"] > 0, t
        for k in (0, 1):                           # no stored state changed, and batch 0 is still the selected one
            e.select_batch(k)
            assert e.export_records() == pr.recs[k]
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ 2. the paired workload
def golden_records():
    b = open(os.path.join(PAIRED, "paired.records.bin"), "rb").read()
    (n,) = struct.unpack_from("<I", b, 0)
    o, recs = 4, []
    for _ in range(n):
        (l,) = struct.unpack_from("<I", b, o)
        recs.append(b[o + 4:o + 4 + l])
        o += 4 + l
    return recs


def workload_body(engine, tmp_path):
    """paired_1.fastq / paired_2.fastq aligned and traced back on the device in batches 0 and 1 against real_db.fasta"""
    g = json.load(open(os.path.join(PAIRED, "paired.json")))["two_files"]
    want = golden_records()
    parts = smr.Index.build(os.path.join(paths.GOLDEN, "real_db.fasta"), 18, 3072.0, 10000, 0)
    slots = max([len(refrun.parse_record(r)["alignv"]) for r in want if r] + [1])
    e = engine()
    reads = []
    try:
        for j, ix in enumerate(parts):
            e.upload_index(ix, j)
        recs = []
        for k in (0, 1):
            e.select_batch(k)
            reads.append(e.upload_fastx(open(os.path.join(PAIRED, "paired_%d.fastq" % (k + 1)), "rb").read(), slots, view=True, keep=True))
            for j, ix in enumerate(parts):
                p = smr.default_params(minimal_score=g["log"]["minimal_score"][0])
                p.index_num, p.part, p.is_last_index_part = 0, j, int(j == len(parts) - 1)
                e.align_part(j, p)
                e.traceback(j, p)
            recs.append(e.export_records())
        e.select_batch(0)
        assert [r for pair in zip(*recs) for r in pair] == want
        n_all = reads[0].count + reads[1].count
        all_len = sum(len(r.record_text(i)[1]) for r in reads for i in range(r.count))
        fr, fq = report.corrected_sizes(g["log"]["K"][0], parts[0].info(), n_all, all_len)
        dbs = {0: (g["log"]["lambda"][0], g["log"]["K"][0], fr, fq)}
        reg = {(0, j): ix for j, ix in enumerate(parts)}
        par = lambda key: smr.default_params(minimal_score=g["log"]["minimal_score"][0])    # noqa: E731
        slot_of = lambda key: key[1]                                                        # noqa: E731
        host = host_rows(tmp_path / "host", reads, recs, True, rows.ALL_COLS, reg, dbs)
        dev = device_rows(tmp_path / "dev", e, True, rows.ALL_COLS, reg, par, dbs, slot_of=slot_of)
        assert host[0].count(b"\n") > 100 and host[1].count(b"\n") > 100
        assert dev[0] == host[0], "aligned.sam differs"
        assert dev[1] == host[1], "aligned.blast differs"
        hp = host_pairwise(tmp_path / "hp", reads, recs, True, reg, dbs)
        assert hp.count(b"Sequence ID: ") > 100
        assert device_pairwise(tmp_path / "dp", e, True, reg, par, dbs, slot_of=slot_of) == hp, "the -blast 0 text differs"
        for k in (0, 1):
            e.select_batch(k)
            assert e.export_records() == recs[k]
    finally:
        e.close()
        for r in reads:
            r.free()
        for ix in parts:
            ix.free()


# ------------------------------------------------------------------------------------------------ 3. the _gz forms
def gz_body(engine, n, fastq):
    pr = Pair(engine, n, fastq, seed=n)
    e = pr.e
    try:
        most = 0
        for key, ix in pr.reg.items():
            p = smr.default_params()
            p.index_num, p.part = key
            lam, K, fr, fq = rows.DB[key[0]]
            for o in rowsgzdev.ROW_OPTS[:3]:
                kw = dict(o, lam=lam, K=K, full_ref=fr, full_read=fq)
                w = "%d pairs, key %s, %s" % (n, key, o)
                sam, blast = e.rows_part_mates(1, 0, p, ix, **kw)
                sam_gz, blast_gz, plain_off = e.rows_part_mates_gz(1, 0, p, ix, **kw)
                t = e.mates_times()
                assert t["d2h"] == 0 and (t["interleave"] > 0 or not (sam or blast)), t
                assert plain_off == [0, len(sam), len(sam) + len(blast)], w
                most = max(most, rowsgzdev.stream_check(e, sam, sam_gz, w + ": SAM"), rowsgzdev.stream_check(e, blast, blast_gz, w + ": BLAST"))
                assert [sam_gz, blast_gz] == e.gzip_lines_batch([sam, blast]), w + ": not the members of gzip_lines_batch"
                assert len(sam_gz) + len(blast_gz) <= e.gzip_lines_bound(len(sam) + len(blast), 2)
                assert e.rows_part_mates_gz(1, 0, p, ix, **kw)[:2] == (sam_gz, blast_gz), w + ": two calls, two outputs"
            kw = dict(lam=lam, K=K, full_ref=fr, full_read=fq)
            text = e.pairwise_part_mates(1, 0, p, ix, **kw)
            gz, plain_bytes = e.pairwise_part_mates_gz(1, 0, p, ix, **kw)
            assert plain_bytes == len(text)
            most = max(most, rowsgzdev.stream_check(e, text, gz, "%d pairs, key %s: pairwise" % (n, key)))
            assert [gz] == e.gzip_lines_batch([text]) and len(gz) <= e.gzip_lines_bound(len(text), 1)
        assert most > 1 or n < 1025, "%d pairs: one member at the most: the cuts were not exercised" % n
        assert e.export_records() == pr.recs[0]
    finally:
        pr.close()


# ------------------------------------------------------------------------------------------------ 4. contract and refusals
def opts(sam=1, blast=1, cols="cigar qcov qstrand"):
    o = capi.RowsOpts()
    o.want_sam, o.want_blast, o.blast_cols = sam, blast, cols.encode()
    o.lam, o.K, o.full_ref_corr, o.full_read_corr = rows.DB[0]
    return o


def rows_call(e, mates, slot, p, ix, o, buf, cap):
    off = (C.c_uint64 * 3)(9, 9, 9)
    need = C.c_uint64(9)
    rc = e.L.smr_rows_part_mates(e.h, mates, slot, C.byref(p) if p is not None else None, ix.h if ix is not None else None, C.byref(o) if o is not None else None,
                                 buf.ctypes.data if buf is not None else None, cap, off, C.byref(need))
    return rc, list(off), need.value


def pair_call(e, mates, slot, p, ix, buf, cap, db=rows.DB[0]):
    need = C.c_uint64(9)
    rc = e.L.smr_pairwise_part_mates(e.h, mates, slot, C.byref(p), ix.h, db[0], db[1], db[2], db[3], buf.ctypes.data if buf is not None else None, cap, C.byref(need))
    return rc, need.value


def contract_body(engine, tmp_path):
    pr = Pair(engine, 130, True, seed=9)
    e, ix, recs, reads = pr.e, pr.ix, pr.recs, pr.reads
    lens = rows.ref_lengths()
    p = smr.default_params()
    db = dict(zip(("lam", "K", "full_ref", "full_read"), rows.DB[0]))
    try:
        plain0 = e.rows_part(0, p, ix, sam=True, blast=True, cols="cigar qcov qstrand", **db)          # the selected batch's own rows, before

        def still_fine():
            assert e.rows_part(0, p, ix, sam=True, blast=True, cols="cigar qcov qstrand", **db) == plain0

        def refused(got, want, *words, call="smr_rows_part_mates"):
            msg = e.L.smr_last_error(e.h).decode()
            assert got == want and call in msg and all(w in msg for w in words), (got, msg)
            assert (buf == 0x5A).all()
            still_fine()

        host = host_rows(tmp_path / "host", reads, recs, True, rows.ALL_COLS, {(0, 0): ix, (0, 1): ix, (1, 0): ix})
        # sizes only; one byte short; exactly `need`; again
        rc, off, need = rows_call(e, 1, 0, p, ix, opts(), None, 0)
        assert rc == 0 and off[0] == 0 and off[2] == need and 0 < off[1] < need
        t = e.mates_times()
        assert t["selected"] > 0 and t["mates"] > 0 and t["interleave"] == 0 and t["d2h"] == 0, t
        buf = np.full(need + 64, 0x5A, dtype=np.uint8)
        rc, off2, need2 = rows_call(e, 1, 0, p, ix, opts(), buf, need - 1)
        assert rc == ERR_CAPACITY and off2 == off and need2 == need
        refused(rc, ERR_CAPACITY)
        rc, off2, need2 = rows_call(e, 1, 0, p, ix, opts(), buf, need)
        assert rc == 0 and off2 == off and (buf[need:] == 0x5A).all()
        first = buf[:need].tobytes()
        assert rows.strip_header(host[0]).startswith(first[:off[1]]) and host[1].startswith(first[off[1]:])
        still_fine()
        buf[:] = 0x5A
        assert rows_call(e, 1, 0, p, ix, opts(), buf, len(buf))[0] == 0 and buf[:need].tobytes() == first and (buf[need:] == 0x5A).all()
        rc, pneed = pair_call(e, 1, 0, p, ix, None, 0)
        assert rc == 0 and pneed > 0
        pbuf = np.full(pneed + 64, 0x5A, dtype=np.uint8)
        assert pair_call(e, 1, 0, p, ix, pbuf, pneed - 1) == (ERR_CAPACITY, pneed) and (pbuf == 0x5A).all()
        assert pair_call(e, 1, 0, p, ix, pbuf, pneed) == (0, pneed) and (pbuf[pneed:] == 0x5A).all()
        ptext = pbuf[:pneed].tobytes()
        pbuf[:] = 0x5A
        assert pair_call(e, 1, 0, p, ix, pbuf, len(pbuf)) == (0, pneed) and pbuf[:pneed].tobytes() == ptext
        buf[:] = 0x5A
        # 1. the call's own arguments
        refused(rows_call(e, 1, 0, p, None, opts(), buf, len(buf))[0], ERR_ARG)
        refused(rows_call(e, 1, 0, p, ix, None, buf, len(buf))[0], ERR_ARG)
        refused(rows_call(e, 1, 64, p, ix, opts(), buf, len(buf))[0], ERR_ARG, "slot")
        for m in (-1, 16, 0):
            refused(rows_call(e, m, 0, p, ix, opts(), buf, len(buf))[0], ERR_ARG, "mates")
            rc, _ = pair_call(e, m, 0, p, ix, buf, len(buf))
            refused(rc, ERR_ARG, "mates", call="smr_pairwise_part_mates")
        refused(rows_call(e, 16, 0, p, ix, opts(sam=0, blast=0), buf, len(buf))[0], ERR_ARG, "mates")          # before the plain call's refusals
        # 2. the plain call's refusals for the selected batch: arguments, state, device-side guards -- each before anything of batch `mates`
        refused(rows_call(e, 2, 0, p, ix, opts(sam=0, blast=0), buf, len(buf))[0], ERR_ARG, "neither")         # (batch 2 holds nothing)
        refused(rows_call(e, 2, 0, p, ix, opts(cols="cigar qcov strand"), buf, len(buf))[0], ERR_ARG, "blast_cols")
        refused(rows_call(e, 2, 5, p, ix, opts(), buf, len(buf))[0], ERR_STATE, "slot empty")
        other = smr.Index.build(golden.inputs("t9")[0], 18, 3072.0, 10000, 0)[0]
        refused(rows_call(e, 2, 0, p, other, opts(), buf, len(buf))[0], ERR_ARG, "resident")
        other.free()
        L = len(reads[0].record_text(0)[1])
        ok = dict(cigar=[(L << 4) | 0], ref_num=0, ref_begin1=0, ref_end1=L - 1, read_begin1=0, read_end1=L - 1, readlen=L, score1=50, part=0, index_num=0, strand=1)
        bad_sets = {"without columns": (dict(ok, cigar=[(0 << 4) | 0]), ERR_ARG), "past its read": (dict(ok, cigar=[((L + 1) << 4) | 0]), ERR_ARG),
                    "ref_num": (dict(ok, ref_num=len(lens)), ERR_ARG), "no CIGAR": (dict(ok, cigar=[]), ERR_STATE)}
        for word, (aln, want) in bad_sets.items():
            e.import_state([rows.record([aln], 6)] + recs[0][1:])
            msg_rc = rows_call(e, 2, 0, p, ix, opts(), buf, len(buf))[0]                   # (the guard of batch 0 speaks before batch 2 is looked at)
            msg = e.L.smr_last_error(e.h).decode()
            assert msg_rc == want and word in msg and "batch" not in msg and "smr_rows_part_mates" in msg, (word, msg_rc, msg)
            assert (buf == 0x5A).all()
            rc, _ = pair_call(e, 2, 0, p, ix, buf, len(buf))
            assert rc == want and "smr_pairwise_part_mates" in e.L.smr_last_error(e.h).decode() and (buf == 0x5A).all()
        e.import_state(recs[0])
        still_fine()
        # 3. batch `mates` without reads, or without their text
        refused(rows_call(e, 2, 0, p, ix, opts(), buf, len(buf))[0], ERR_STATE, "SMR_FASTX_KEEP", "batch 2")
        rc, _ = pair_call(e, 2, 0, p, ix, buf, len(buf))
        refused(rc, ERR_STATE, "SMR_FASTX_KEEP", "batch 2", call="smr_pairwise_part_mates")
        # (the _gz forms refuse in the same places, under their own names)
        gz_off, plain_off, gneed, gplain = (C.c_uint64 * 3)(), (C.c_uint64 * 3)(), C.c_uint64(9), C.c_uint64(9)
        rc = e.L.smr_rows_part_mates_gz(e.h, 16, 0, C.byref(p), ix.h, C.byref(opts()), buf.ctypes.data, len(buf), gz_off, plain_off, C.byref(gneed))
        refused(rc, ERR_ARG, "mates", call="smr_rows_part_mates_gz")
        rc = e.L.smr_rows_part_mates_gz(e.h, 2, 0, C.byref(p), ix.h, C.byref(opts()), buf.ctypes.data, len(buf), gz_off, plain_off, C.byref(gneed))
        refused(rc, ERR_STATE, "SMR_FASTX_KEEP", "batch 2", call="smr_rows_part_mates_gz")
        rc = e.L.smr_pairwise_part_mates_gz(e.h, 2, 0, C.byref(p), ix.h, *rows.DB[0], buf.ctypes.data, len(buf), C.byref(gplain), C.byref(gneed))
        refused(rc, ERR_STATE, "SMR_FASTX_KEEP", "batch 2", call="smr_pairwise_part_mates_gz")
        assert list(gz_off) == [0, 0, 0] and gneed.value == 0 and gplain.value == 0
        plain = smr.Reads.from_seqs([reads[1].record_text(i)[1] for i in range(5)])
        e.select_batch(3)
        e.upload_reads(plain, 6)
        e.select_batch(0)
        plain.free()
        refused(rows_call(e, 3, 0, p, ix, opts(), buf, len(buf))[0], ERR_STATE, "SMR_FASTX_KEEP", "batch 3")          # (before its unequal count)
        # 4. unequal read counts; FASTA against FASTQ
        text5, recs5, slots5 = rows.craft(5, True, lens, seed=3)
        e.select_batch(3)
        r5 = e.upload_fastx(text5, slots5, view=True, keep=True)
        e.select_batch(0)
        refused(rows_call(e, 3, 0, p, ix, opts(), buf, len(buf))[0], ERR_ARG, "130 reads, 5 mates")
        rc, _ = pair_call(e, 3, 0, p, ix, buf, len(buf))
        refused(rc, ERR_ARG, "130 reads, 5 mates", call="smr_pairwise_part_mates")
        r5.free()
        texta, recsa, slotsa = rows.craft(130, False, lens, seed=4)
        e.select_batch(3)
        ra = e.upload_fastx(texta, slotsa, view=True, keep=True)
        e.import_state(recsa)
        e.select_batch(0)
        refused(rows_call(e, 3, 0, p, ix, opts(), buf, len(buf))[0], ERR_ARG, "FASTA reads with FASTQ mates")
        ra.free()
        # 5. the device-side guards for batch `mates`: the message names the batch
        L1 = len(reads[1].record_text(0)[1])
        ok1 = dict(ok, cigar=[(L1 << 4) | 0], ref_end1=L1 - 1, read_end1=L1 - 1, readlen=L1)
        bad_sets = {"without columns": (dict(ok1, cigar=[(0 << 4) | 0]), ERR_ARG), "past its read": (dict(ok1, cigar=[((L1 + 1) << 4) | 0]), ERR_ARG),
                    "past its read or its reference": (dict(ok1, ref_begin1=lens[0] - L1 + 1), ERR_ARG),
                    "ref_num": (dict(ok1, ref_num=len(lens)), ERR_ARG), "no CIGAR": (dict(ok1, cigar=[]), ERR_STATE)}
        for word, (aln, want) in bad_sets.items():
            e.select_batch(1)
            e.import_state([rows.record([aln], 6)] + recs[1][1:])
            e.select_batch(0)
            refused(rows_call(e, 1, 0, p, ix, opts(), buf, len(buf))[0], want, word, "batch 1")
            rc, _ = pair_call(e, 1, 0, p, ix, buf, len(buf))
            refused(rc, want, word, "batch 1", call="smr_pairwise_part_mates")
        e.select_batch(1)
        e.import_state(recs[1])
        e.select_batch(0)
        # two empty batches
        e.select_batch(4)
        e.upload_fastx(b"", 6, view=True, keep=True).free()
        e.select_batch(5)
        e.upload_fastx(b"", 6, view=True, keep=True).free()
        assert rows_call(e, 4, 0, p, ix, opts(), buf, len(buf)) == (0, [0, 0, 0], 0) and pair_call(e, 4, 0, p, ix, buf, len(buf)) == (0, 0)
        assert (buf == 0x5A).all()
        e.select_batch(0)
        # the context goes on working: the same bytes, and no stored state has changed
        assert rows_call(e, 1, 0, p, ix, opts(), buf, len(buf))[0] == 0 and buf[:need].tobytes() == first and (buf[need:] == 0x5A).all()
        still_fine()
        for k in (0, 1):
            e.select_batch(k)
            assert e.export_records() == recs[k]
    finally:
        pr.close()
