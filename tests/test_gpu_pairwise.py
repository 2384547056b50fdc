"""smr_pairwise_part: the BLAST-like pairwise text (-blast 0) of one (index, part), guarded, sized and written by kernels (csrc/smr_pairwise.hpp)
from the kept text, the packed letters, the stored alignments with their CIGARs and the part's reference letters.

The yardstick of every test is the host writer (smr_report_add of a report opened with blast_pairwise, pinned to the reference's own files by
test_reports_cpu.py) or a file the unmodified reference wrote (tests/golden/reports2), never the code under test.

1. explicit CIGARs (helpers/pairwise.py): alignments of 1 .. 121 columns, gaps that straddle, end at and begin at a chunk boundary, chunks made
   of insertion or deletion only, CIGARs that begin and end with a gap, chunk numbers that cross 9 / 99 / 999, soft clips, both strands, N /
   lowercase / U, a reference with N, a reference beyond the names table, a score that needs the large table;
2. the crafted state of helpers/rows.py at 1 .. 1025 reads: block counts per key, blocks at all four byte phases, a block longer than the LDS
   window with more than 64 operations;
3. whole golden workloads, aligned and traced on the device;
4. the four files the reference wrote for `-blast 0`;
5. the contract and the refusals of include/smr_hip.h;
6. the report side (no device).

test_emu_pairwise.py runs the same bodies on the kernel emulator."""
import ctypes as C
import os

import numpy as np
import pytest

import sortmerna_amd as smr
from sortmerna_amd import report
from helpers import fastx, golden, pairwise, refrun, rows
from test_gpu_rows import COUNTS, WORKLOADS, crafted_engine, syn_part
from test_gpu_state_import import case_setup, engine

ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -4, -5
FIXTURES = ["t0", "t9", "syn_default", "real_default"]
REPORTS2 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reports2")


def default_params(key):
    return smr.default_params()


# ------------------------------------------------------------------------------------------------ 1. column cases
def columns_body(tmp_path):
    ix, lens = syn_part()
    refs = [s for _, s, _ in fastx.read_fastx(rows.SYN_DB)]
    text, recs, slots = pairwise.column_batch(refs)
    reg = {key: ix for key in rows.KEYS}
    e = engine()
    try:
        e.upload_index(ix, 0)
        reads = e.upload_fastx(text, slots, view=True, keep=True)
        assert reads.count == len(pairwise.COLUMN_CASES)
        e.import_state(recs)
        streams = {}
        host = pairwise.host_file(tmp_path / "host", reads, recs, False, reg)
        dev = pairwise.device_file(tmp_path / "dev", e, False, reg, default_params, streams=streams)
        reads.free()
    finally:
        e.close()
    # what the expected text must hold for the comparison to show anything
    blocks = {b["query"]: b for b in pairwise.parse(host)}
    assert sorted(blocks) == sorted(c[0] for c in pairwise.COLUMN_CASES)
    for n in (1, 59, 60, 61, 119, 120, 121):
        assert [len(c[1]) for c in blocks["m%d" % n]["chunks"]] == [60] * ((n - 1) // 60) + [(n - 1) % 60 + 1]
    ch = blocks["i_straddle"]["chunks"]
    assert ch[0][1].endswith("---") and ch[0][1][56] != "-" and ch[1][1].startswith("--") and ch[1][1][2] != "-" and ch[0][3].endswith("   ") and ch[1][3].startswith("  ")
    ch = blocks["d_straddle"]["chunks"]
    assert ch[0][5].endswith("---") and ch[0][5][56] != "-" and ch[1][5].startswith("--") and ch[1][5][2] != "-"
    assert blocks["i_ends60"]["chunks"][0][1].endswith("-----") and "-" not in blocks["i_ends60"]["chunks"][1][1]
    assert blocks["d_ends60"]["chunks"][0][5].endswith("-----") and "-" not in blocks["d_ends60"]["chunks"][1][5]
    assert "-" not in blocks["i_begins60"]["chunks"][0][1] and blocks["i_begins60"]["chunks"][1][1].startswith("-----")
    assert "-" not in blocks["d_begins60"]["chunks"][0][5] and blocks["d_begins60"]["chunks"][1][5].startswith("-----")
    assert blocks["i_begins60b"]["chunks"][0][1].endswith("-") and blocks["i_begins60b"]["chunks"][1][1].startswith("----")
    assert blocks["d_begins60b"]["chunks"][0][5].endswith("-") and blocks["d_begins60b"]["chunks"][1][5].startswith("----")
    first, letters, last, marks = blocks["i_chunk"]["chunks"][1][:4]                   # a chunk made of insertions: "last" is one less than "first"
    assert letters == "-" * 60 and marks == " " * 60 and last == first - 1 and len(blocks["i_chunk"]["chunks"]) == 3
    assert blocks["i_first_chunk"]["chunks"][0][:3] == (1, "-" * 60, 0)
    ch = blocks["d_chunk"]["chunks"]
    assert ch[1][5] == "-" * 60 and ch[1][6] == ch[1][4] - 1 and ch[1][2] == ch[1][0] + 59 and len(ch) == 3
    for name in ("i_ends", "i_ends_rev"):
        assert blocks[name]["chunks"][0][1].startswith("---") and blocks[name]["chunks"][-1][1].endswith("----")
    assert blocks["d_ends"]["chunks"][0][5].startswith("---") and blocks["d_ends"]["chunks"][-1][5].endswith("----")
    firsts = {c[0] for b in blocks.values() for c in b["chunks"]}
    lasts = {c[2] for b in blocks.values() for c in b["chunks"]}
    assert {9, 10, 99, 100, 999, 1000} <= firsts and {99, 100, 999, 1000} <= lasts
    assert blocks["clip"]["chunks"][0][4] == 8 and blocks["clip_rev"]["chunks"][0][4] == 12             # the first Query number behind a soft clip
    assert {b["strand"] for b in blocks.values()} == {"+", "-"}
    for name in ("letters", "letters_rev"):
        assert "N" in "".join(c[5] for c in blocks[name]["chunks"])
    assert all(any("*" in c[3] for c in b["chunks"]) for name, b in blocks.items() if name.startswith("digits"))
    assert blocks["other_part"]["ref"] == "*" and blocks["other_index"]["ref"] != "*"                   # a reference beyond the names table
    assert blocks["high_score"]["score"] == 60000
    assert [len(c[1]) for c in blocks["zero_ops"]["chunks"]] == [60, 20] and [len(c[1]) for c in blocks["zero_ops_rev"]["chunks"]] == [60, 32]
    assert dev == host, "aligned.blast differs"
    assert host == b"".join(streams[k] for k in sorted(streams)) and all(streams[k] for k in rows.KEYS)


@pytest.mark.gpu
def test_explicit_cigars_equal_the_host_writer(tmp_path):
    columns_body(tmp_path)


def n_reference_body(tmp_path):
    """a database whose references hold N: it shows in a Target line, N against N is marked '|' as the host marks it, N against a letter '*'"""
    rng = np.random.Generator(np.random.PCG64(5))
    refs = []
    for k in range(2):
        s = list("".join("ACGT"[int(c)] for c in rng.integers(0, 4, 320)))
        for pos in (10, 40, 41, 69, 70, 200):
            s[pos] = "N"
        refs.append("".join(s))
    db = tmp_path / "n_db.fasta"
    db.write_text("".join(">nref%d some words\n%s\n" % (k, s) for k, s in enumerate(refs)))
    ix = smr.Index.build(str(db), 18, 3072.0, 10000, 0)[0]
    cases = [("n_n", [(80, 0)], 10, 0, 1, (0, 0), None, "N"), ("n_n_rev", [(30, 0), (2, 1), (100, 0)], 35, 0, 0, (0, 0), None, ""),
             ("n_gap", [(25, 0), (10, 2), (40, 0)], 10, 4, 1, (0, 0), None, "")]
    text, recs, slots = pairwise.column_batch(refs, cases)
    reg = {(0, 0): ix}
    e = engine()
    try:
        e.upload_index(ix, 0)
        reads = e.upload_fastx(text, slots, view=True, keep=True)
        e.import_state(recs)
        host = pairwise.host_file(tmp_path / "host", reads, recs, False, reg)
        dev = pairwise.device_file(tmp_path / "dev", e, False, reg, default_params)
        reads.free()
    finally:
        e.close()
        ix.free()
    blocks = {b["query"]: b for b in pairwise.parse(host)}
    t, m, q = blocks["n_n"]["chunks"][0][1], blocks["n_n"]["chunks"][0][3], blocks["n_n"]["chunks"][0][5]
    assert (t[0], m[0], q[0]) == ("N", "|", "N") and (t[30], m[30]) == ("N", "*") and q[30] != "N"
    assert all("N" in "".join(c[1] for c in b["chunks"]) for b in blocks.values())
    assert "N" in blocks["n_gap"]["chunks"][0][1][25:35] and blocks["n_gap"]["chunks"][0][5][25:35] == "-" * 10      # an N of the reference at a deletion
    assert dev == host, "aligned.blast differs"


@pytest.mark.gpu
def test_a_reference_with_n_equals_the_host_writer(tmp_path):
    n_reference_body(tmp_path)


# ------------------------------------------------------------------------------------------------ 2. crafted state
def crafted_body(n, fastq, tmp_path, seed=1, long_read=False):
    e, reads, recs, reg = crafted_engine(n, fastq, seed, long_read)
    try:
        streams = {}
        host = pairwise.host_file(tmp_path / "host", reads, recs, fastq, reg)
        dev = pairwise.device_file(tmp_path / "dev", e, fastq, reg, default_params, streams=streams, feed=(reads, recs))
        assert dev == host, "%d reads, fastq=%s: aligned.blast differs" % (n, fastq)
        # per (index, part): one block per alignment of that key, and the streams in key order are the file
        parsed = [refrun.parse_record(r) for r in recs if r]
        for key in rows.KEYS:
            want = sum(1 for p in parsed for a in p["alignv"] if (a["index_num"], a["part"]) == key)
            assert streams[key].count(b"Sequence ID: ") == want, key
        assert host == b"".join(streams[k] for k in sorted(streams))
        if n >= 1023:
            blocks = pairwise.parse(streams[(0, 0)])
            assert {b["start"] % 4 for b in blocks} == {0, 1, 2, 3}                    # blocks begin at all four byte phases
            assert {b["strand"] for b in blocks} == {"+", "-"} and any(b["score"] == 60000 for b in blocks)
            assert any("-" in c[1] for b in blocks for c in b["chunks"]) and any("-" in c[5] for b in blocks for c in b["chunks"])
            assert any("N" in c[5] for b in blocks for c in b["chunks"])
            assert all(b["ref"] == "*" for b in pairwise.parse(streams[(0, 1)]))
        if long_read:
            blocks = pairwise.parse(streams[(0, 0)])
            sizes = np.diff([b["start"] for b in blocks] + [len(streams[(0, 0)])])
            longest = max(parsed, key=lambda p: p["alignv"][0]["readlen"])["alignv"]
            assert sizes.max() > 4096 + 64 and sizes.min() < 1000 and max(len(a["cigar"]) for a in longest) > 64      # longer than the LDS window (ROWS_WINDOW), more than one wave of operations
    finally:
        e.close()
        reads.free()


@pytest.mark.gpu
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("n", COUNTS)
def test_crafted_state_equals_the_host_writer(n, fastq, tmp_path):
    crafted_body(n, fastq, tmp_path, seed=n)


@pytest.mark.gpu
def test_a_block_longer_than_the_window_next_to_short_blocks(tmp_path):
    crafted_body(70, True, tmp_path, seed=5, long_read=True)


# ------------------------------------------------------------------------------------------------ 3. whole workloads
def corrected_dbs(cs):
    g = cs["golden"]
    dbs = {}
    for k, x in enumerate(cs["idx"]):
        fr, fq = report.corrected_sizes(g["log"]["K"][k], x["parts"][0].info(), g["readstats"]["all_reads_count"], g["readstats"]["all_reads_len"])
        dbs[k] = (g["log"]["lambda"][k], g["log"]["K"][k], fr, fq)
    return dbs


def workload_body(case, tmp_path, mode=0):
    cs = case_setup(case)
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
        dbs = corrected_dbs(cs)
        host = pairwise.host_file(tmp_path / "host", reads, recs, False, reg, dbs)
        dev = pairwise.device_file(tmp_path / "dev", e, False, reg, lambda key: cs["plist"][key[0]], dbs, slot_of=lambda key, ix: slot[key])
        assert host.count(b"Sequence ID: ") > 3
        assert dev == host, "%s: aligned.blast differs" % case
        assert e.export_records() == recs                            # no stored state changed
        reads.free()
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", WORKLOADS)
def test_workload_text_equals_the_host_loop(case, tmp_path):
    workload_body(case, tmp_path)


# ------------------------------------------------------------------------------------------------ 4. the reference's own files
def fixture_body(case, tmp_path):
    g = golden.load()[case]
    db, rd, _ = golden.inputs(case)
    recs = golden.records(case)
    parts = smr.Index.build(db, 18, 3072.0, 10000, 0)
    slots = max([1] + [len(refrun.parse_record(r)["alignv"]) for r in recs if r])
    fr, fq = report.corrected_sizes(g["log"]["K"][0], parts[0].info(), g["readstats"]["all_reads_count"], g["readstats"]["all_reads_len"])
    dbs = {0: (g["log"]["lambda"][0], g["log"]["K"][0], fr, fq)}
    reg = {(0, k): ix for k, ix in enumerate(parts)}
    e = engine()
    try:
        for k, ix in enumerate(parts):
            e.upload_index(ix, k)
        reads = e.upload_fastx(open(rd, "rb").read(), slots, view=True, keep=True)
        assert reads.count == len(recs)
        e.import_state(recs)
        host = pairwise.host_file(tmp_path / "host", reads, recs, False, reg, dbs)
        dev = pairwise.device_file(tmp_path / "dev", e, False, reg, default_params, dbs, slot_of=lambda key, ix: key[1], feed=(reads, recs))
        reads.free()
    finally:
        e.close()
    got = dev.decode().split("\n")
    exp = open(os.path.join(REPORTS2, case + ".pairwise.txt")).read().split("\n")
    assert len(got) == len(exp) > 4
    for a, b in zip(got, exp):
        if a.startswith("Score: "):               # the fixtures' lambda and K are known to six digits only: the rule of test_reports_cpu.py
            fa, fb = a.split("\t"), b.split("\t")
            assert fa[0] == fb[0] and fa[2] == fb[2], (a, b)
            ea, eb = float(fa[1].split(": ")[1]), float(fb[1].split(": ")[1])
            assert abs(ea - eb) <= 1.2e-2 * eb, (a, b)
        else:
            assert a == b, (a, b)
    assert dev == host, "%s: aligned.blast differs from the host writer's" % case


@pytest.mark.gpu
@pytest.mark.parametrize("case", FIXTURES)
def test_the_device_text_equals_the_reference_file(case, tmp_path):
    fixture_body(case, tmp_path)


# ------------------------------------------------------------------------------------------------ 5. contract and refusals
def call(e, slot, p, ix, buf, cap, db=rows.DB[0]):
    need = C.c_uint64(9)
    rc = e.L.smr_pairwise_part(e.h, slot, C.byref(p), ix.h, db[0], db[1], db[2], db[3], buf.ctypes.data if buf is not None else None, cap, C.byref(need))
    return rc, need.value


def refused(e, rc, want, *words):
    msg = e.L.smr_last_error(e.h).decode()
    assert rc == want and "smr_pairwise_part" in msg and all(w in msg for w in words), (rc, msg)


def contract_body(tmp_path):
    ix, lens = syn_part()
    e, reads, recs, reg = crafted_engine(130, True, seed=9)
    p = smr.default_params()
    try:
        before = e.export_records()
        want = {}
        pairwise.device_file(tmp_path / "x", e, True, {(0, 0): ix}, default_params, streams=want)
        host = pairwise.host_file(tmp_path / "host", reads, recs, True, reg)
        assert host.startswith(want[(0, 0)]) and want[(0, 0)]
        # the size only
        rc, need = call(e, 0, p, ix, None, 0)
        assert rc == 0 and need == len(want[(0, 0)])
        # one byte short: refused, the buffer untouched, the size valid
        buf = np.full(need + 64, 0x5A, dtype=np.uint8)
        rc, need2 = call(e, 0, p, ix, buf, need - 1)
        refused(e, rc, ERR_CAPACITY)
        assert (buf == 0x5A).all() and need2 == need
        # exactly `need` bytes, nothing behind them
        rc, need2 = call(e, 0, p, ix, buf, need)
        assert rc == 0 and need2 == need and (buf[need:] == 0x5A).all() and buf[:need].tobytes() == want[(0, 0)]
        # again: the same bytes
        buf[:] = 0x5A
        assert call(e, 0, p, ix, buf, len(buf)) == (0, need) and buf[:need].tobytes() == want[(0, 0)] and (buf[need:] == 0x5A).all()
        t = e.pairwise_times()
        assert sorted(t) == ["d2h", "sizes", "stats", "write"] and all(v >= 0 for v in t.values())
        # no alignment of the key: nothing
        buf[:] = 0x5A
        p.index_num, p.part = 3, 2
        assert call(e, 0, p, ix, buf, len(buf)) == (0, 0) and (buf == 0x5A).all()
        p.index_num, p.part = 0, 0
        # not the part in the slot
        other = smr.Index.build(golden.inputs("t9")[0], 18, 3072.0, 10000, 0)[0]
        refused(e, call(e, 0, p, other, buf, len(buf))[0], ERR_ARG, "slot")
        other.free()
        # (an e-value or bit-score text too long for the table: `%.3g` of a double and a 32-bit integer never are, so no input reaches that refusal)
        # state the host writer would read out of bounds for, each counted on the device before any byte is written
        L = len(reads.record_text(0)[1])
        ok = dict(cigar=[(L << 4) | 0], ref_num=0, ref_begin1=0, ref_end1=L - 1, read_begin1=0, read_end1=L - 1, readlen=L, score1=50, part=0, index_num=0, strand=1)
        bad_sets = {"without columns": dict(ok, cigar=[(0 << 4) | 0]),
                    "past its read": dict(ok, cigar=[((L + 1) << 4) | 0]),
                    "past its read or its reference": dict(ok, ref_begin1=lens[0] - L + 1),
                    "ref_num": dict(ok, ref_num=len(lens))}
        for what, aln in bad_sets.items():
            e.import_state([rows.record([aln], 6)] + recs[1:])
            refused(e, call(e, 0, p, ix, buf, len(buf))[0], ERR_ARG, what)
        # an alignment of the part without its CIGAR
        e.import_state([rows.record([dict(ok, cigar=[])], 6)] + recs[1:])
        refused(e, call(e, 0, p, ix, buf, len(buf))[0], ERR_STATE, "CIGAR")
        assert (buf == 0x5A).all()
        # a batch without kept text
        e.import_state(recs)
        e.select_batch(1)
        plain = smr.Reads.from_seqs([reads.record_text(i)[1] for i in range(reads.count)])
        e.upload_reads(plain, 6)
        e.import_state(recs)
        refused(e, call(e, 0, p, ix, buf, len(buf))[0], ERR_STATE, "SMR_FASTX_KEEP")
        assert (buf == 0x5A).all()
        plain.free()
        e.select_batch(0)
        # the context goes on working, and no stored state has changed
        assert call(e, 0, p, ix, buf, len(buf)) == (0, need) and buf[:need].tobytes() == want[(0, 0)]
        assert e.export_records() == before == recs
    finally:
        e.close()
        reads.free()


@pytest.mark.gpu
def test_contract_and_refusals(tmp_path):
    contract_body(tmp_path)


# ------------------------------------------------------------------------------------------------ 6. the report side
HDR, SEQ = ">r1 words", "ACGTACGTACGTACGTACGTAAAACCCCGGGGTTTT"


def _one_record(ix_lens):
    L = len(SEQ)
    return rows.record([dict(cigar=[(L << 4) | 0], ref_num=0, ref_begin1=5, ref_end1=5 + L - 1, read_begin1=0, read_end1=L - 1, readlen=L, score1=50, part=0, index_num=0, strand=1)], 1)


def report_side_body(tmp_path):
    ix, lens = syn_part()
    reg = {(0, 0): ix}
    text = b"Sequence ID: x\nQuery ID: y\n"
    rep = rows.open_report(tmp_path / "a", False, None, reg)                               # SAM only: not opened for pairwise
    assert rep.L.smr_report_add_pairwise(rep.h, 0, 0, text, len(text)) == ERR_ARG and "smr_report_add_pairwise" in rep.L.smr_report_last_error(rep.h).decode()
    assert rep.L.smr_report_add_pairwise(rep.h, 0, 0, None, 0) == 0                        # an empty stream is nothing
    rep.close()
    rep = pairwise.open_report(tmp_path / "b", False, reg, tabular=True)                   # opened for tabular too: the host writes no pairwise text
    assert rep.L.smr_report_add_pairwise(rep.h, 0, 0, text, len(text)) == ERR_ARG
    rep.close()
    assert pairwise.blast_file(tmp_path / "b") == b""
    rep = pairwise.open_report(tmp_path / "c", False, reg)
    assert rep.L.smr_report_add_pairwise(rep.h, 0, 1, text, len(text)) == ERR_ARG          # not registered
    assert rep.L.smr_report_add_pairwise(rep.h, 0, 0, text, len(text)) == 0
    rep.add_pairwise(0, 0, b"more\n")
    rep.close()
    assert pairwise.blast_file(tmp_path / "c") == text + b"more\n"
    # skip_pairwise leaves SAM alone; skip_rows leaves pairwise alone
    rec = _one_record(lens)
    out = {}
    for what in ("plain", "skip_pairwise", "skip_rows"):
        rep = pairwise.open_report(tmp_path / what, False, reg, sam=True)
        if what != "plain":
            getattr(rep, what)()
        rep.add(HDR, SEQ, None, rec)
        rep.close()
        out[what] = (pairwise.blast_file(tmp_path / what), rows.strip_header(open(tmp_path / what / "aligned.sam", "rb").read()))
    assert out["plain"][0].startswith(b"Sequence ID: ") and out["plain"][1].startswith(b"r1\t0\t")
    assert out["skip_pairwise"] == (b"", out["plain"][1])
    assert out["skip_rows"] == (out["plain"][0], b"")


def test_report_add_pairwise_refusals_and_the_two_skips(tmp_path):
    report_side_body(tmp_path)
