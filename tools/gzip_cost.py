"""What gzipping aligned.fq.gz / other.fq.gz of a batch costs on the device (smr_fastx_split_gz into a pinned buffer + smr_report_add_fastx_gz:
the DEFLATE kernels of csrc/smr_gzip.hpp, only gzip members cross the bus) against the host's way under zip_out (smr_fastx_split into a pinned
buffer + smr_report_add_fastx, which sends every byte through gzwrite at zlib's default level on one thread), on the same reads: a FASTQ file of
single-end reads of 150 nt, uploaded once with SMR_FASTX_KEEP | SMR_FASTX_VIEW, `hit` drawn at --hit-rate.  Both paths write to --dir (default
/dev/shm).  The host path is too slow to repeat at 8 M reads, so it is timed at --host-reads, where the device path is timed as well and the
sizes are set next to zlib level 6 and level 1 of the same bytes; the device path alone is then timed at --reads.  Per path: wall time per call
after one warm-up call, median of the repeats; for the device path the HIP-event times of smr_gzip_times beside it.  Needs a GPU.

    python tools/gzip_cost.py --reads 8000000 --out profiles/gzip_cost.log
"""
import argparse
import ctypes as C
import gzip
import os
import shutil
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sortmerna_amd as smr  # noqa: E402
from sortmerna_amd import capi  # noqa: E402
from sortmerna_amd.report import Report  # noqa: E402
from fastx_pack_cost import write_files  # noqa: E402


def timed(fn, repeats):
    fn()                                                        # warm-up: buffers at their size, code objects loaded
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def zsize(parts, level):
    n = 0
    for p in parts:
        z = zlib.compressobj(level, zlib.DEFLATED, 31)
        n += len(z.compress(p)) + len(z.flush())
    return n


def run(e, L, torch, lines, work, n_reads, a, with_host, repeats):
    d = os.path.join(work, "n%d" % n_reads)
    os.makedirs(d)
    fq, fa = write_files(d, n_reads, a.read_len, 1234)
    os.remove(fa)
    reads = e.upload_fastx(fq, 1, view=True, keep=True)
    assert e.fastx_info()[0] == 0, "the host parser ran"
    os.remove(fq)
    hit = (np.random.default_rng(5).random(n_reads) < a.hit_rate).astype(np.uint8)
    o = capi.FxSplitOpts(0, 0, 0, 0, 0, 1, 1)
    off, gz_off, need = (C.c_uint64 * 9)(), (C.c_uint64 * 9)(), C.c_uint64()
    assert L.smr_fastx_split(e.h, -1, C.byref(o), hit.ctypes.data, None, 0, off, C.byref(need)) == 0
    plain = need.value
    lines.append("%d reads: %d bytes of aligned.fq + other.fq, %d reads drawn as hits" % (n_reads, plain, int(hit.sum())))
    cap = int(L.smr_gzip_bound(plain, plain // int(L.smr_gzip_chunk()) + 8))
    pinned = torch.empty(max(cap, plain) + 64, dtype=torch.uint8, pin_memory=True)
    outs = {k: os.path.join(d, k) for k in ("host", "device")}
    for p in outs.values():
        os.makedirs(p)
    stages = {}

    def host():
        rep = Report(outs["host"], True, fastx=True, other=True, zip_out=True)
        t0 = time.perf_counter()
        assert L.smr_fastx_split(e.h, -1, C.byref(o), hit.ctypes.data, pinned.data_ptr(), pinned.numel(), off, C.byref(need)) == 0, L.smr_last_error(e.h)
        t1 = time.perf_counter()
        assert L.smr_report_add_fastx(rep.h, pinned.data_ptr(), off) == 0
        rep.close()
        stages["h_split"], stages["h_write"] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    def device():
        rep = Report(outs["device"], True, fastx=True, other=True, zip_out=True)
        t0 = time.perf_counter()
        assert L.smr_fastx_split_gz(e.h, -1, C.byref(o), hit.ctypes.data, pinned.data_ptr(), cap, gz_off, off, C.byref(need)) == 0, L.smr_last_error(e.h)
        t1 = time.perf_counter()
        assert L.smr_report_add_fastx_gz(rep.h, pinned.data_ptr(), gz_off) == 0
        rep.close()
        stages["d_split"], stages["d_write"], stages["d_bytes"] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, need.value

    paths = [("(b) device: fastx_split_gz (pinned) + report_add_fastx_gz", device, repeats)]
    if with_host:
        paths.insert(0, ("(a) host: fastx_split (pinned) + report_add_fastx under zip_out", host, max(1, min(repeats, 2))))
    for what, fn, rp in paths:
        med, lo, hi = timed(fn, rp)
        row = "  %-66s %10.1f ms [%.1f .. %.1f]  %7.2f M reads/s, %7.1f MB/s of plain text (median of %d)" % (what, med * 1e3, lo * 1e3, hi * 1e3, n_reads / med * 1e-6, plain / med * 1e-6, rp)
        if what.startswith("(a)"):
            row += "\n      last call: smr_fastx_split %.1f ms wall; smr_report_add_fastx (gzwrite) + close %.1f ms" % (stages["h_split"], stages["h_write"])
        else:
            row += "\n      last call: smr_fastx_split_gz %.1f ms wall (HIP events: %s), %d gzip bytes out (%.3f of plain); smr_report_add_fastx_gz + close %.1f ms" % (
                stages["d_split"], ", ".join("%s %.1f ms" % kv for kv in e.gzip_times().items()), stages["d_bytes"], stages["d_bytes"] / plain, stages["d_write"])
        lines.append(row)
        print(row, flush=True)
    if with_host:
        names = ("aligned.fq.gz", "other.fq.gz")
        texts = [gzip.open(os.path.join(outs["host"], f), "rb").read() for f in names]
        assert texts == [gzip.open(os.path.join(outs["device"], f), "rb").read() for f in names], "the two paths wrote files that inflate differently"
        hs, ds = [[os.path.getsize(os.path.join(outs[k], f)) for f in names] for k in ("host", "device")]
        z6, z1 = zsize(texts, 6), zsize(texts, 1)
        lines.append("  files inflate to the same text.  sizes (aligned + other): host path %d, device %d; zlib level 6 %d, level 1 %d of the same bytes -> device / level 6 = %.2f, device / level 1 = %.2f"
                     % (sum(hs), sum(ds), z6, z1, sum(ds) / z6, sum(ds) / z1))
    reads.free()
    del pinned
    shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8000000)
    ap.add_argument("--host-reads", type=int, default=500000, help="the count at which the host path (and the device path next to it) is timed")
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--hit-rate", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch                                                # (the pinned buffer)
    e = smr.Engine(0)                                           # raises without a GPU
    L = capi.load()
    lines = ["gzip_cost: FASTQ reads of %d nt, single-end, hit rate %.2f, gzip files written to %s, wall time per call after one warm-up [min .. max]; chunk %d bytes"
             % (a.read_len, a.hit_rate, a.dir, int(L.smr_gzip_chunk())),
             "the host path (zlib level 6 on one thread) is too slow to repeat at %d reads: it is timed at %d reads, the device path at both counts" % (a.reads, a.host_reads)]
    work = tempfile.mkdtemp(prefix="gz_cost_", dir=a.dir)
    try:
        run(e, L, torch, lines, work, a.host_reads, a, True, a.repeats)
        if a.reads != a.host_reads:
            run(e, L, torch, lines, work, a.reads, a, False, a.repeats)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    e.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
