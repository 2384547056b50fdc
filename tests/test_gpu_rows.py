"""smr_rows_part: the rows of aligned.sam and of the BLAST tabular report of one (index, part), counted, sized and written by kernels
(csrc/smr_rows.hpp) from the kept text, the packed letters, the stored alignments with their CIGARs and the part's reference letters.

The yardstick of every test is the host writer (smr_report_add, pinned to the reference's own files by test_reports_cpu.py), never the code
under test: the same reads and records go through it into a temporary directory and the files are compared for equality.

1. crafted state (helpers/rows.py): both strands, soft clips in front / behind / both / none, CIGARs with I and D and multi-digit lengths, reads
   with N, lowercase and U, headers with a space, a tab before any space, `>>` / `@@`, nothing behind the id, FASTA and FASTQ, the quality
   parity of two and three alignments of one key with alignments of other keys between them, reads without alignments, every order and subset
   of the optional BLAST columns; 1, 63, 64, 65, 1023, 1024, 1025 reads; rows at all four byte phases; a 5 kb read with more than 64 operations;
2. whole golden workloads with several alignments per read and several keys;
3. the number formatter against Python's '%.3g' of the same double;
4. the guards and refusals of include/smr_hip.h.

test_emu_rows.py runs the same bodies on the kernel emulator."""
import ctypes as C
import itertools

import numpy as np
import pytest

import sortmerna_amd as smr
from sortmerna_amd import capi, report
from helpers import golden, refrun, rows
from test_gpu_state_import import case_setup, engine

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -4, -5
COUNTS = [1, 63, 64, 65, 1023, 1024, 1025]
WORKLOADS = ["syn_default", "syn_all", "syn_best3", "two_db_default", "two_db_all", "syn_multipart"]
COL_SETS = [list(p) for r in range(0, 4) for p in itertools.permutations(rows.ALL_COLS, r)]

_part = {}


def syn_part():
    """a small real index part (tests/golden/syn_db.fasta), built once per process"""
    if "ix" not in _part:
        _part["ix"] = smr.Index.build(rows.SYN_DB, 18, 3072.0, 10000, 0)[0]
        _part["lens"] = rows.ref_lengths()
    return _part["ix"], _part["lens"]


def crafted_engine(n, fastq, seed=1, long_read=False):
    """-> (engine with the part in slot 0 and the crafted state imported, the host parser's view of the reads, records, registry)"""
    ix, lens = syn_part()
    text, recs, slots = rows.craft(n, fastq, lens, seed=seed, long_read=long_read)
    e = engine()
    e.upload_index(ix, 0)
    reads = e.upload_fastx(text, slots, view=True, keep=True)
    assert reads.count == n
    e.import_state(recs)
    return e, reads, recs, {key: ix for key in rows.KEYS}


def rows_equal(e, reads, recs, reg, fastq, cols, tmp_path, what, streams=None):
    host = rows.host_files(tmp_path / "host", reads, recs, fastq, cols, reg)
    dev = rows.device_files(tmp_path / "dev", e, fastq, cols, reg, lambda key: smr.default_params(), streams=streams)
    assert dev[0] == host[0], "%s: aligned.sam differs" % what
    assert dev[1] == host[1], "%s: aligned.blast differs" % what
    return host


# ------------------------------------------------------------------------------------------------ 1. crafted state
def crafted_body(n, fastq, tmp_path, seed=1, long_read=False, cols=rows.ALL_COLS):
    e, reads, recs, reg = crafted_engine(n, fastq, seed, long_read)
    try:
        streams = {}
        host = rows_equal(e, reads, recs, reg, fastq, cols, tmp_path, "%d reads, fastq=%s" % (n, fastq), streams)
        # per (index, part): the device's stream holds one row per alignment of that key, and the streams in key order are the file
        parsed = [refrun.parse_record(r) for r in recs if r]
        for key in rows.KEYS:
            want = sum(1 for p in parsed for a in p["alignv"] if (a["index_num"], a["part"]) == key)
            assert streams[key][0].count(b"\n") == want and streams[key][1].count(b"\n") == want, key
        assert rows.strip_header(host[0]) == b"".join(streams[k][0] for k in sorted(streams))
        assert host[1] == b"".join(streams[k][1] for k in sorted(streams))
        if n >= 1023:
            for s in streams[(0, 0)]:                 # rows begin at all four byte phases of each stream
                starts = np.cumsum([0] + [len(l) + 1 for l in s.split(b"\n")[:-1]])[:-1]
                assert {int(x) % 4 for x in starts} == {0, 1, 2, 3}
            sam = streams[(0, 0)][0].split(b"\n")
            assert any(l.split(b"\t")[1] == b"16" for l in sam[:-1]) and any(l.split(b"\t")[1] == b"0" for l in sam[:-1])
            assert any(b"I" in l.split(b"\t")[5] and b"D" in l.split(b"\t")[5] for l in sam[:-1])
            assert any(b"N" in l.split(b"\t")[9] for l in sam[:-1])
            assert any(l.split(b"\t")[2] == b"*" for l in streams[(0, 1)][0].split(b"\n")[:-1])      # a reference beyond the names table
        if long_read:
            longest = max(streams[(0, 0)][0].split(b"\n"), key=len)
            fields = longest.split(b"\t")
            assert len(longest) > 8192 and sum(fields[5].count(c) for c in (b"M", b"I", b"D")) > 64      # longer than the LDS window, more than one wave of operations
            assert min(len(l) for l in streams[(0, 0)][1].split(b"\n")[:-1]) < 100
    finally:
        e.close()
        reads.free()


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("n", COUNTS)
def test_crafted_rows_equal_the_host_writer(n, fastq, tmp_path):
    crafted_body(n, fastq, tmp_path, seed=n)


def test_a_row_longer_than_the_window_next_to_short_rows(tmp_path):
    crafted_body(70, True, tmp_path, seed=5, long_read=True)


def columns_body(tmp_path):
    e, reads, recs, reg = crafted_engine(130, True, seed=3)
    try:
        for j, cols in enumerate(COL_SETS):
            rows_equal(e, reads, recs, reg, True, cols, tmp_path / str(j), "columns %s" % cols)
        rows_equal(e, reads, recs, reg, True, None, tmp_path / "sam_only", "SAM only")
    finally:
        e.close()
        reads.free()


def test_blast_columns_in_every_order_and_subset(tmp_path):
    assert len(COL_SETS) == 16
    columns_body(tmp_path)


# ------------------------------------------------------------------------------------------------ 2. whole workloads
def workload_body(case, tmp_path, mode=0):
    cs = case_setup(case)
    g = cs["golden"]
    data = open(golden.inputs(case)[1], "rb").read()
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
        recs = e.export_records()
        assert recs == golden.records(case)
        reg = {(k, part): ix for k, part, ix in steps}
        slot = {(k, part): j for j, (k, part, ix) in enumerate(steps)}
        dbs = {}
        for k, x in enumerate(cs["idx"]):
            fr, fq = report.corrected_sizes(g["log"]["K"][k], x["parts"][0].info(), g["readstats"]["all_reads_count"], g["readstats"]["all_reads_len"])
            dbs[k] = (g["log"]["lambda"][k], g["log"]["K"][k], fr, fq)
        host = rows.host_files(tmp_path / "host", reads, recs, False, rows.ALL_COLS, reg, dbs)
        dev = rows.device_files(tmp_path / "dev", e, False, rows.ALL_COLS, reg, lambda key: cs["plist"][key[0]], dbs, slot_of=lambda key, ix: slot[key])
        assert host[0].count(b"\n") > 3 and host[1]
        assert dev[0] == host[0], "%s: aligned.sam differs" % case
        assert dev[1] == host[1], "%s: aligned.blast differs" % case
        assert e.export_records() == recs                            # no stored state changed
        reads.free()
    finally:
        e.close()


@pytest.mark.parametrize("case", WORKLOADS)
def test_workload_rows_equal_the_host_loop(case, tmp_path):
    workload_body(case, tmp_path)


# ------------------------------------------------------------------------------------------------ 3. the formatter
def fmt_pairs(max_den):
    den = np.concatenate([np.full(d + 1, d, dtype=np.uint32) for d in list(range(1, max_den + 1)) + list(range(4998, 5004))])
    num = np.concatenate([np.arange(d + 1, dtype=np.uint32) for d in list(range(1, max_den + 1)) + list(range(4998, 5004))])
    return num, den


def fmt_body(max_den):
    num, den = fmt_pairs(max_den)
    e = engine()
    try:
        got = e.rows_fmt_batch(num, den)
    finally:
        e.close()
    want = ["%.3g" % (int(a) / int(b) * 100) for a, b in zip(num, den)]
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, "%d of %d differ, first 100 * %d / %d: %r against %r" % (len(bad), len(want), num[bad[0]], den[bad[0]], got[bad[0]], want[bad[0]])


def test_the_device_formatter_prints_what_printf_prints():
    fmt_body(2000)


# ------------------------------------------------------------------------------------------------ 4. guards and refusals
def call(e, slot, p, ix, o, buf, cap):
    off = (C.c_uint64 * 3)(9, 9, 9)
    need = C.c_uint64(9)
    rc = e.L.smr_rows_part(e.h, slot, C.byref(p), ix.h, C.byref(o), buf.ctypes.data if buf is not None else None, cap, off, C.byref(need))
    return rc, list(off), need.value


def opts(sam=1, blast=1, cols="cigar qcov qstrand"):
    o = capi.RowsOpts()
    o.want_sam, o.want_blast, o.blast_cols = sam, blast, cols.encode()
    o.lam, o.K, o.full_ref_corr, o.full_read_corr = rows.DB[0]
    return o


def guards_body(tmp_path):
    ix, lens = syn_part()
    e, reads, recs, reg = crafted_engine(130, True, seed=9)
    p = smr.default_params()
    try:
        before = e.export_records()
        host = rows.host_files(tmp_path / "host", reads, recs, True, rows.ALL_COLS, reg)
        want_sam = rows.strip_header(host[0])
        # sizes only
        rc, off, need = call(e, 0, p, ix, opts(), None, 0)
        assert rc == 0 and off[0] == 0 and off[2] == need and need > 0
        # one byte short: refused, the buffer untouched, the sizes valid
        buf = np.full(need + 64, 0x5A, dtype=np.uint8)
        rc, off2, need2 = call(e, 0, p, ix, opts(), buf, need - 1)
        assert rc == ERR_CAPACITY and (buf == 0x5A).all() and off2 == off and need2 == need
        # exactly `need` bytes, nothing behind them
        rc, off2, need2 = call(e, 0, p, ix, opts(), buf, need)
        assert rc == 0 and off2 == off and (buf[need:] == 0x5A).all()
        first = buf[:need].tobytes()
        assert want_sam.startswith(first[:off[1]]) and first[:off[1]].endswith(b"\n")
        # again: the same bytes
        buf[:] = 0x5A
        assert call(e, 0, p, ix, opts(), buf, len(buf))[0] == 0 and buf[:need].tobytes() == first and (buf[need:] == 0x5A).all()
        # the refusals of the arguments
        buf[:] = 0x5A
        assert call(e, 0, p, ix, opts(sam=0, blast=0), buf, len(buf))[0] == ERR_ARG                       # neither stream
        assert call(e, 0, p, ix, opts(cols="cigar qcov strand"), buf, len(buf))[0] == ERR_ARG             # an unknown word
        other = smr.Index.build(golden.inputs("t9")[0], 18, 3072.0, 10000, 0)[0]
        assert call(e, 0, p, other, opts(), buf, len(buf))[0] == ERR_ARG                                  # not the part in the slot
        other.free()
        assert "slot" in e.L.smr_last_error(e.h).decode()
        # state the host writer would read out of bounds for, each checked on the device before any byte is written
        L = len(reads.record_text(0)[1])
        ok = dict(cigar=[(L << 4) | 0], ref_num=0, ref_begin1=0, ref_end1=L - 1, read_begin1=0, read_end1=L - 1, readlen=L, score1=50, part=0, index_num=0, strand=1)
        bad_sets = {"a CIGAR without columns": dict(ok, cigar=[(0 << 4) | 0]),
                    "a CIGAR past its read": dict(ok, cigar=[((L + 1) << 4) | 0]),
                    "a CIGAR past its reference": dict(ok, ref_begin1=lens[0] - L + 1),
                    "ref_num beyond the part": dict(ok, ref_num=len(lens))}
        for what, aln in bad_sets.items():
            e.import_state([rows.record([aln], 6)] + recs[1:])
            rc, _, _ = call(e, 0, p, ix, opts(), buf, len(buf))
            assert rc == ERR_ARG, what
        # an alignment of the part without its CIGAR
        e.import_state([rows.record([dict(ok, cigar=[])], 6)] + recs[1:])
        assert call(e, 0, p, ix, opts(), buf, len(buf))[0] == ERR_STATE
        assert "CIGAR" in e.L.smr_last_error(e.h).decode()
        assert (buf == 0x5A).all()
        # a batch without kept text
        e.import_state(recs)
        e.select_batch(1)
        plain = smr.Reads.from_seqs([reads.record_text(i)[1] for i in range(reads.count)])
        e.upload_reads(plain, 6)
        e.import_state(recs)
        assert call(e, 0, p, ix, opts(), buf, len(buf))[0] == ERR_STATE and "SMR_FASTX_KEEP" in e.L.smr_last_error(e.h).decode()
        assert (buf == 0x5A).all()
        plain.free()
        e.select_batch(0)
        # the context goes on working, and no stored state has changed
        assert call(e, 0, p, ix, opts(), buf, len(buf))[0] == 0 and buf[:need].tobytes() == first
        assert e.export_records() == before == recs
    finally:
        e.close()
        reads.free()


def test_guards_and_refusals(tmp_path):
    guards_body(tmp_path)


def report_side_body(tmp_path):
    ix, _ = syn_part()
    rep = rows.open_report(tmp_path / "a", True, None, {(0, 0): ix})                 # SAM only
    try:
        off = (C.c_uint64 * 3)
        assert rep.L.smr_report_add_rows(rep.h, 0, 0, b"ab\ncd\n", off(0, 3, 6)) == ERR_ARG        # BLAST rows, no BLAST report
        assert rep.L.smr_report_add_rows(rep.h, 0, 0, b"ab\ncd\n", off(0, 3, 2)) == ERR_ARG        # offsets decrease
        assert rep.L.smr_report_add_rows(rep.h, 0, 1, b"ab\ncd\n", off(0, 3, 3)) == ERR_ARG        # not registered
        assert rep.L.smr_report_add_rows(rep.h, 0, 0, b"ab\ncd\n", off(0, 3, 3)) == 0
    finally:
        rep.close()
    assert rows.strip_header(open(tmp_path / "a" / "aligned.sam", "rb").read()) == b"ab\n"
