"""What writing aligned.fq / other.fq of a batch costs on the device (smr_fastx_split into a pinned buffer + smr_report_add_fastx) against the
host's way (smr_results_fetch, then per read smr_reads_record_text twice and smr_report_add: the loop of examples/smr_align.cpp, run in native
code by tools/fastx_split_host_loop.cpp), on the same reads: a FASTQ file of --reads single-end reads of 150 nt, uploaded once with
SMR_FASTX_KEEP | SMR_FASTX_VIEW, `hit` drawn at --hit-rate.  Both paths write to --dir (default /dev/shm).  Per path: wall time per call after
one warm-up call, median of --repeats; for the device path the HIP-event times of its stages beside it.  Needs a GPU and g++.

    python tools/fastx_split_cost.py --reads 8000000 --out profiles/fastx_split_cost.log
"""
import argparse
import ctypes as C
import os
import shutil
import statistics
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sortmerna_amd as smr  # noqa: E402
from sortmerna_amd import build, capi  # noqa: E402
from sortmerna_amd.report import Report  # noqa: E402
from fastx_pack_cost import write_files  # noqa: E402

HIT_RECORD = struct.pack("<6I3BHiIQIIQ", 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 16, 0, 0, 0)      # a hit without stored alignments


def host_loop_library(d):
    so = os.path.join(d, "libfxs_host_loop.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tools", "fastx_split_host_loop.cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", build.LIBDIR, "-lsmr_hip", "-Wl,-rpath," + build.LIBDIR, "-o", so])
    lib = C.CDLL(so)
    lib.fxs_host_loop.restype = C.c_int
    lib.fxs_host_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_uint64]
    return lib


def timed(fn, repeats):
    fn()                                                        # warm-up: buffers at their size, code objects loaded
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--hit-rate", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch                                                # (the pinned buffer)
    e = smr.Engine(0)                                           # raises without a GPU
    L = capi.load()
    lines = ["fastx_split_cost: %d FASTQ reads of %d nt, single-end, hit rate %.2f, files written to %s, median of %d calls after one warm-up [min .. max]"
             % (a.reads, a.read_len, a.hit_rate, a.dir, a.repeats)]
    work = tempfile.mkdtemp(prefix="fxs_cost_", dir=a.dir)
    code = tempfile.mkdtemp(prefix="fxs_cost_")                # (a memory file system is often mounted noexec)
    try:
        host_lib = host_loop_library(code)
        fq, fa = write_files(work, a.reads, a.read_len, 1234)
        os.remove(fa)
        size = os.path.getsize(fq)
        reads = e.upload_fastx(fq, 1, view=True, keep=True)
        assert e.fastx_info()[0] == 0, "the host parser ran"
        hit = (np.random.default_rng(5).random(a.reads) < a.hit_rate).astype(np.uint8)
        lines.append("reads.fq: %d bytes; %d of %d reads drawn as hits" % (size, int(hit.sum()), a.reads))
        outs = {k: os.path.join(work, k) for k in ("host", "device")}
        for p in outs.values():
            os.makedirs(p)

        def host():
            rep = Report(outs["host"], True, fastx=True, other=True)
            rc = host_lib.fxs_host_loop(e.h, reads.h, rep.h, 1, hit.ctypes.data, HIT_RECORD, len(HIT_RECORD))
            assert rc == 0, rc
            rep.close()

        o = capi.FxSplitOpts(0, 0, 0, 0, 0, 1, 1)
        off, need = (C.c_uint64 * 9)(), C.c_uint64()
        assert L.smr_fastx_split(e.h, -1, C.byref(o), hit.ctypes.data, None, 0, off, C.byref(need)) == 0
        pinned = torch.empty(need.value + 64, dtype=torch.uint8, pin_memory=True)
        stages = {}

        def device():
            rep = Report(outs["device"], True, fastx=True, other=True)
            t0 = time.perf_counter()
            rc = L.smr_fastx_split(e.h, -1, C.byref(o), hit.ctypes.data, pinned.data_ptr(), pinned.numel(), off, C.byref(need))
            assert rc == 0, e.L.smr_last_error(e.h)
            t1 = time.perf_counter()
            rc = L.smr_report_add_fastx(rep.h, pinned.data_ptr(), off)
            assert rc == 0, rc
            rep.close()
            stages["split"], stages["write"] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        for what, fn in [("(a) host: fetch + record_text x 2 + report_add per read", host), ("(b) device: fastx_split (pinned) + report_add_fastx", device)]:
            med, lo, hi = timed(fn, a.repeats)
            row = "  %-56s %9.1f ms [%.1f .. %.1f]  %6.1f M reads/s" % (what, med * 1e3, lo * 1e3, hi * 1e3, a.reads / med * 1e-6)
            if what.startswith("(b)"):
                row += "\n      last call: smr_fastx_split %.1f ms wall (HIP events: %s), %d bytes out; smr_report_add_fastx + close %.1f ms" % (
                    stages["split"], ", ".join("%s %.1f ms" % kv for kv in e.fastx_split_times().items()), need.value, stages["write"])
            lines.append(row)
            print(row, flush=True)
        same = all(open(os.path.join(outs["host"], f), "rb").read() == open(os.path.join(outs["device"], f), "rb").read() for f in ("aligned.fq", "other.fq"))
        assert same and sorted(os.listdir(outs["host"])) == sorted(os.listdir(outs["device"])), "the two paths wrote different files"
        lines.append("  files equal (aligned.fq %d bytes, other.fq %d bytes)" % tuple(os.path.getsize(os.path.join(outs["device"], f)) for f in ("aligned.fq", "other.fq")))
        reads.free()
    finally:
        shutil.rmtree(work, ignore_errors=True)
        shutil.rmtree(code, ignore_errors=True)
    e.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
