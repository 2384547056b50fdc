"""The timing contract of the device report writers (include/smr_hip.h: smr_rows_times, smr_pairwise_times, smr_otu_times,
smr_fastx_split_times, smr_gzip_times) on one tiny workload, for test_gpu_stage_times.py / test_emu_stage_times.py.  TEST INFRASTRUCTURE ONLY.

What is pinned is when the times of a family are written, not how large they are: a sizes-only call leaves the stages it never reached at
exactly 0.0, a full call leaves every entry finite and not negative, and a call that returns before its first stage (an empty batch), or that
belongs to another family (smr_fastx_denovo shares the split's kernels, not its clock), leaves the previous call's values alone.

smr_gzip_times[2] (bit packing) is finite and not negative on a sizes-only call, not 0.0 as the header has it: gz_run records the events on
both sides of the encode launch it skips, so the entry holds the distance of two neighbouring events.  It was so before the stage clock
(csrc/smr_stage.hpp) took the events over; pinned as found."""
import ctypes as C
import math

import numpy as np

import sortmerna_amd as smr
from sortmerna_amd import capi, report
from . import golden

CASE = "syn_default"
N_READS = 48


def _sane(times, zero=()):
    vals = list(times.values())
    print("stage times:", times)
    assert all(math.isfinite(v) and v >= 0.0 for v in vals), times
    for k in zero:
        assert vals[k] == 0.0, (k, times)        # exactly: the stage never ran


def body(engine, case_setup):
    """engine() -> an Engine on the library under test; case_setup(case) -> the golden case of test_gpu_state_import"""
    cs = case_setup(CASE)
    g = cs["golden"]
    assert len(cs["steps"]) == 1
    k, part, ix = cs["steps"][0]
    p = cs["plist"][k]
    p.index_num, p.part, p.is_last_index_part = k, part, 1
    text = open(golden.inputs(CASE)[1], "rb").read()
    text = b">".join(text.split(b">")[:N_READS + 1])
    lam, K = g["log"]["lambda"][k], g["log"]["K"][k]
    fr, fq = report.corrected_sizes(K, cs["idx"][k]["parts"][0].info(), g["readstats"]["all_reads_count"], g["readstats"]["all_reads_len"])
    e = engine()
    try:
        L, h = e.L, e.h
        e.upload_index(ix, 0)
        reads = e.upload_fastx(text, cs["slots"], view=True, keep=True)
        assert reads.count == N_READS
        e.align_part(0, p)
        e.traceback(0, p)
        e.idcov_part(0, p, 0.0, 0.0)
        need = C.c_uint64(0)

        # ---- smr_rows_part
        o = capi.RowsOpts()
        o.want_sam, o.want_blast, o.blast_cols = 1, 1, b"cigar qcov qstrand"
        o.lam, o.K, o.full_ref_corr, o.full_read_corr = lam, K, fr, fq
        off3 = (C.c_uint64 * 3)()
        assert L.smr_rows_part(h, 0, C.byref(p), ix.h, C.byref(o), None, 0, off3, C.byref(need)) == 0 and need.value > 0
        _sane(e.rows_times(), zero=(2, 3))
        buf = np.zeros(need.value, dtype=np.uint8)
        assert L.smr_rows_part(h, 0, C.byref(p), ix.h, C.byref(o), buf.ctypes.data, len(buf), off3, C.byref(need)) == 0
        rows_full = e.rows_times()
        _sane(rows_full)

        # ---- smr_pairwise_part
        args = (h, 0, C.byref(p), ix.h, float(lam), float(K), int(fr), int(fq))
        assert L.smr_pairwise_part(*args, None, 0, C.byref(need)) == 0 and need.value > 0
        _sane(e.pairwise_times(), zero=(2, 3))
        buf = np.zeros(need.value, dtype=np.uint8)
        assert L.smr_pairwise_part(*args, buf.ctypes.data, len(buf), C.byref(need)) == 0
        _sane(e.pairwise_times())
        assert e.rows_times() == rows_full             # (the two calls share device buffers, not times)

        # ---- smr_otu_part
        need2, any_ = (C.c_uint64 * 2)(), C.c_int(0)
        args = (h, 0, C.byref(p), ix.h, 0.0, 0.0)
        assert L.smr_otu_part(*args, None, 0, None, 0, need2, C.byref(any_)) == 0 and need2[1] > 0
        _sane(e.otu_times(), zero=(3, 4))
        buf = np.zeros(need2[0], dtype=np.uint8)
        grp = np.zeros(need2[1], dtype=smr.engine.OTU_GROUP)
        assert L.smr_otu_part(*args, buf.ctypes.data, len(buf), grp.ctypes.data, len(grp), need2, C.byref(any_)) == 0
        _sane(e.otu_times())

        # ---- smr_fastx_split
        fo = capi.FxSplitOpts(0, 0, 0, 0, 0, 1, 1)
        off9 = (C.c_uint64 * 9)()
        assert L.smr_fastx_split(h, -1, C.byref(fo), None, None, 0, off9, C.byref(need)) == 0 and need.value > 0
        _sane(e.fastx_split_times(), zero=(2, 3))
        buf = np.zeros(need.value, dtype=np.uint8)
        assert L.smr_fastx_split(h, -1, C.byref(fo), None, buf.ctypes.data, len(buf), off9, C.byref(need)) == 0
        split_full = e.fastx_split_times()
        _sane(split_full)
        plain = buf.tobytes()

        # ---- smr_gzip_batch
        offs = (C.c_uint64 * 2)(0, len(plain))
        gz_off = (C.c_uint64 * 2)()
        src = np.frombuffer(plain, dtype=np.uint8)
        assert L.smr_gzip_batch(h, src.ctypes.data, offs, 1, None, 0, gz_off, C.byref(need)) == 0 and need.value > 0
        _sane(e.gzip_times(), zero=(3, 4))             # ([2]: see the module's text)
        buf = np.zeros(need.value, dtype=np.uint8)
        assert L.smr_gzip_batch(h, src.ctypes.data, offs, 1, buf.ctypes.data, len(buf), gz_off, C.byref(need)) == 0
        _sane(e.gzip_times())

        # ---- smr_fastx_denovo keeps no times, and leaves the split's alone
        e.fastx_denovo()
        assert e.fastx_split_times() == split_full

        # ---- smr_rows_part on an empty batch returns before its clock starts
        e.select_batch(1)
        none = e.upload_fastx(b"", cs["slots"], view=True, keep=True)
        assert none.count == 0
        assert L.smr_rows_part(h, 0, C.byref(p), ix.h, C.byref(o), None, 0, off3, C.byref(need)) == 0 and need.value == 0
        assert e.rows_times() == rows_full
        none.free()
        e.select_batch(0)
        reads.free()
    finally:
        e.close()
