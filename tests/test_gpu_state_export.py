"""smr_state_export: the records of a whole batch sized and serialised on the device, back to back with an offsets array -- the counterpart of
smr_state_import and the bulk form of smr_results_fetch + smr_result_record.

1. the writer at its boundaries: crafted records (every byte phase of a record start, CIGARs of 0, 1, 70 and 130 words, 1 .. slots alignments)
   imported, exported, compared with their concatenation -- offsets and bytes; batches of 0, 1, 63, 64, 65 and 700 reads;
2. the guards of include/smr_hip.h: nothing behind `need` is touched, a short buffer is refused untouched, sizes only, wrong n, no batch;
3. real runs: export_records() == records() after every (index, part), before and after smr_traceback, and the reference's records at the end;
4. after the %id / %coverage pass the records carry the counters;
5. a run split between two contexts through export -> import gives the unsplit run's records and counters.

Every equality is byte equality.  test_emu_state_export.py runs the same bodies on the emulator, where device memory lies between guard pages."""
import ctypes as C

import numpy as np
import pytest

import sortmerna_amd as smr
from helpers import golden, otu, refrun
from test_gpu_state_import import SPLIT_CASES, case_setup, crafted_batch, engine, run_steps, same_records, unsplit_counters

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -4, -5
REAL_CASES = list(dict.fromkeys(SPLIT_CASES + ["two_db_all"]))
SMALL_N = [0, 1, 63, 64, 65]


def concat(recs):
    off = np.zeros(len(recs) + 1, dtype=np.uint64)
    if recs:
        off[1:] = np.cumsum([len(r) for r in recs], dtype=np.uint64)
    return b"".join(recs), off


def export_equals(e, recs, what):
    blob, off = e.export_state()
    raw, want = concat(recs)
    assert off.dtype == np.uint64 and blob.dtype == np.uint8
    assert off.tolist() == want.tolist(), "%s: offsets differ" % what
    if blob.tobytes() != raw:
        got = [blob[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(recs))]
        same_records(got, recs, what)
    assert blob.tobytes() == raw, what


# ------------------------------------------------------------------------------------------------ 1. boundaries, through import
def boundaries_body(n=700):
    slots = 4
    seqs, full = crafted_batch(n=n, slots=slots)
    reads = smr.Reads.from_seqs(seqs)
    if n >= 700:
        parsed = [refrun.parse_record(r) for r in full]
        starts = np.cumsum([0] + [len(r) for r in full])[:-1]
        assert {int(s) % 4 for s in starts} == {0, 1, 2, 3}                       # a record starts at every byte phase
        assert {0, 1, 70, 130} <= {len(a["cigar"]) for p in parsed for a in p["alignv"]}
        assert any(len(p["alignv"]) == slots for p in parsed)
        assert n % 64 and n > 2 * 256                                             # a last partial wave, several blocks of four waves
    sets = {"every read": full,
            "every third read": [full[i] if i % 3 == 0 else b"" for i in range(n)],
            "first and last only": [full[i] if i in (0, n - 1) else b"" for i in range(n)],
            "no record": [b""] * n}
    e = engine()
    try:
        e.upload_reads(reads, slots)
        for what, recs in sets.items():
            e.import_state(recs)
            export_equals(e, recs, "%d reads, %s" % (n, what))
            assert e.export_records() == recs
    finally:
        e.close()
        reads.free()


def test_the_writer_at_its_boundaries():
    boundaries_body()


@pytest.mark.parametrize("n", SMALL_N)
def test_small_batches(n):
    boundaries_body(n)


# ------------------------------------------------------------------------------------------------ 2. guards
def guards_body():
    slots = 4
    seqs, recs = crafted_batch(n=130, slots=slots)
    reads = smr.Reads.from_seqs(seqs)
    n = len(seqs)
    raw, want = concat(recs)
    e = engine()
    try:
        off = np.zeros(n + 1, dtype=np.uint64)
        need = C.c_uint64(7)
        assert e.L.smr_state_export(e.h, None, 0, off.ctypes.data, n, C.byref(need)) == ERR_STATE          # no batch
        e.upload_reads(reads, slots)
        e.import_state(recs)
        # sizes only
        assert e.L.smr_state_export(e.h, None, 0, off.ctypes.data, n, C.byref(need)) == 0
        assert need.value == len(raw) and off.tolist() == want.tolist()
        assert e.L.smr_state_export(e.h, None, 0, off.ctypes.data, n, None) == 0
        need.value = 0
        assert e.L.smr_state_export(e.h, None, 0, None, n, C.byref(need)) == 0 and need.value == len(raw)
        # a larger buffer: the tail stays as it was
        buf = np.full(len(raw) + 64, 0x5A, dtype=np.uint8)
        off[:] = 0
        assert e.L.smr_state_export(e.h, buf.ctypes.data, len(buf), off.ctypes.data, n, C.byref(need)) == 0
        assert buf[:len(raw)].tobytes() == raw and (buf[len(raw):] == 0x5A).all() and off.tolist() == want.tolist()
        # an exact one, with the tail behind it watched
        buf[:] = 0x5A
        assert e.L.smr_state_export(e.h, buf.ctypes.data, len(raw), off.ctypes.data, n, C.byref(need)) == 0
        assert buf[:len(raw)].tobytes() == raw and (buf[len(raw):] == 0x5A).all()
        # one byte short
        buf[:] = 0x5A
        off[:] = 0
        need.value = 0
        assert e.L.smr_state_export(e.h, buf.ctypes.data, len(raw) - 1, off.ctypes.data, n, C.byref(need)) == ERR_CAPACITY
        assert (buf == 0x5A).all() and off.tolist() == want.tolist() and need.value == len(raw)
        # a wrong n
        for bad_n in (n - 1, n + 1):
            big = np.zeros(n + 2, dtype=np.uint64)
            assert e.L.smr_state_export(e.h, buf.ctypes.data, len(buf), big.ctypes.data, bad_n, C.byref(need)) == ERR_ARG
        assert (buf == 0x5A).all()
        # the context goes on working
        export_equals(e, recs, "after the refusals")
        e.fetch()
        same_records(e.records(), recs, "fetch after the refusals")
    finally:
        e.close()
        reads.free()


def test_guards():
    guards_body()


# ------------------------------------------------------------------------------------------------ 3. real runs
def real_run_body(case, mode=0):
    cs = case_setup(case)
    steps = cs["steps"]
    e = engine(mode)
    try:
        e.upload_reads(cs["reads"], cs["slots"])
        export_equals(e, [b""] * len(cs["seqs"]), "%s: a fresh upload" % case)
        for j, (k, part, ix) in enumerate(steps):
            p = cs["plist"][k]
            p.index_num, p.part, p.is_last_index_part = k, part, int(j == len(steps) - 1)
            e.upload_index(ix, 0)
            e.align_part(0, p)
            got = e.export_records()                       # before smr_traceback: this part's alignments have no CIGAR yet
            e.fetch()
            same_records(got, e.records(), "%s: step %d before the traceback" % (case, j))
            e.traceback(0, p)
            got = e.export_records()
            e.fetch()
            same_records(got, e.records(), "%s: step %d" % (case, j))
            e.unload_index(0)
        assert any(got)
        same_records(got, golden.records(case), "%s: the reference's records" % case)
    finally:
        e.close()


@pytest.mark.parametrize("case", REAL_CASES)
def test_export_equals_fetch_and_records_at_every_step(case):
    real_run_body(case)


# ------------------------------------------------------------------------------------------------ 4. after the id / coverage pass
def after_idcov_body(tmpdir, case="syn"):
    e = engine()
    try:
        recs, tot, keep = otu.run(e, case, tmpdir)
        try:
            assert any(r and any(r[8:24]) for r in recs), "no record carries an id / coverage counter"
            same_records(e.export_records(), recs, "%s after smr_idcov_part" % case)
            same_records(recs, otu.records(case), "%s: the reference's records after denovo_stats" % case)
        finally:
            otu.free(keep)
    finally:
        e.close()


def test_records_after_the_id_coverage_pass_carry_the_counters(tmp_path):
    after_idcov_body(tmp_path)


# ------------------------------------------------------------------------------------------------ 5. a split run through export
def split_body(case, k=1, mode=0):
    cs = case_setup(case)
    steps, n_db = cs["steps"], len(cs["idx"])
    assert 0 < k < len(steps)
    a = engine(mode)
    try:
        a.upload_reads(cs["reads"], cs["slots"])
        run_steps(a, cs, steps[:k], [False] * k)
        blob, off = a.export_state()
        ctr = a.counters(n_db)
    finally:
        a.close()
    assert len(blob) and int(off[-1]) == len(blob)
    b = engine(mode)
    try:
        b.upload_reads(cs["reads"], cs["slots"])
        b.import_state((blob, off))
        b.import_counters(ctr, n_db)
        run_steps(b, cs, steps[k:], [i == len(steps) - 1 for i in range(k, len(steps))])
        got_recs = b.export_records()
        b.fetch()
        same_records(b.records(), golden.records(case), "%s split at %d through export" % (case, k))
        same_records(got_recs, golden.records(case), "%s split at %d, exported" % (case, k))
        got = b.counters(n_db)
    finally:
        b.close()
    g = cs["golden"]
    assert got == unsplit_counters(case, mode)
    assert got["num_aligned"] == g["readstats"]["num_aligned"] and got["reads_matched_per_db"] == g["readstats"]["reads_matched_per_db"]


@pytest.mark.parametrize("case", REAL_CASES)
def test_a_run_split_through_export_equals_the_unsplit_run(case):
    split_body(case)
