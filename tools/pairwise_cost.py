"""What writing the BLAST pairwise report (aligned.blast of -blast 0) of a batch costs on the device (smr_pairwise_part into a pinned buffer +
smr_report_add_pairwise) against the host's way (smr_results_fetch, then per read smr_reads_record_text, smr_result_record and smr_report_add:
the loop of examples/smr_align.cpp, run in native code by tools/rows_host_loop.cpp), on the same batch: a FASTQ file of --reads single-end reads of
150 nt, 10 % of them sampled from a synthetic database of --db-nt letters (the bench workload's generator), uploaded once with SMR_FASTX_KEEP |
SMR_FASTX_VIEW, aligned and traced back once.  Both paths write to --dir (default /dev/shm).  Per path: wall time per call after one warm-up
call, median of --repeats; for the device path the HIP-event times of its stages (smr_pairwise_times) beside it.  The two files are compared in
the same run.  Needs a GPU and g++.

    python tools/pairwise_cost.py --reads 8000000 --out profiles/pairwise_cost.log
"""
import argparse
import ctypes as C
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sortmerna_amd as smr  # noqa: E402
from sortmerna_amd import build, capi, report, synth  # noqa: E402
from fastx_split_cost import timed  # noqa: E402

GUMBEL = (0.618874, 0.343238)          # scheme 2 / -3 / 5 / 2, near-uniform background (bench.py)


def host_loop_library(d):
    so = os.path.join(d, "librows_host_loop.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tools", "rows_host_loop.cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", build.LIBDIR, "-lsmr_hip", "-Wl,-rpath," + build.LIBDIR, "-o", so])
    lib = C.CDLL(so)
    lib.rows_host_loop.restype = C.c_int
    lib.rows_host_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--db-nt", type=int, default=2000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch                                                # (the pinned buffer)
    e = smr.Engine(0)                                           # raises without a GPU
    L = capi.load()
    lines = ["pairwise_cost: %d FASTQ reads of %d nt, single-end, 10 %% sampled from a synthetic database of %d nt, BLAST pairwise (-blast 0) written to %s, "
             "median of %d calls after one warm-up [min .. max]" % (a.reads, a.read_len, a.db_nt, a.dir, a.repeats)]
    work = tempfile.mkdtemp(prefix="pairwise_cost_", dir=a.dir)
    code = tempfile.mkdtemp(prefix="pairwise_cost_")               # (a memory file system is often mounted noexec)
    try:
        host_lib = host_loop_library(code)
        db = os.path.join(work, "db.fasta")
        synth.make_db(db, a.db_nt, seed=42)
        codes, offs = synth.load_db_codes(db)
        fq = os.path.join(work, "reads.fq")
        synth.write_fastq(fq, synth.make_reads_fast(codes, offs, a.reads, read_len=a.read_len, frac_db=0.10, seed=1234, sub=0.005, indel=0.0001, n_rate=0.001))
        parts = smr.Index.build(db, 18, 3072.0, 10000, 0)
        assert len(parts) == 1
        ix = parts[0]
        reads = e.upload_fastx(fq, 1, view=True, keep=True)
        assert e.fastx_info()[0] == 0, "the host parser ran"
        lam, K = GUMBEL
        p = smr.default_params(minimal_score=smr.minimal_score(lam, K, ix.info(), reads.count, reads.total_len))
        p.index_num, p.part, p.is_last_index_part = 0, 0, 1
        e.upload_index(ix, 0)
        e.align_part(0, p)
        e.traceback(0, p)
        fr, fqc = report.corrected_sizes(K, ix.info(), reads.count, reads.total_len)
        aligned = e.counters(1)["num_aligned"]
        lines.append("reads.fq: %d bytes; %d of %d reads aligned (%.1f %%)" % (os.path.getsize(fq), aligned, a.reads, 100.0 * aligned / a.reads))
        outs = {k: os.path.join(work, k) for k in ("host", "device")}
        for d in outs.values():
            os.makedirs(d)

        def open_report(d):
            rep = report.Report(d, True, fastx=False, other=False, blast_pairwise=True)
            rep.set_db(0, lam, K, fr, fqc)
            rep.set_part(0, 0, ix)
            return rep

        def host():
            rep = open_report(outs["host"])
            rc = host_lib.rows_host_loop(e.h, reads.h, rep.h, 1)
            assert rc == 0, rc
            rep.close()

        need = C.c_uint64()
        assert L.smr_pairwise_part(e.h, 0, C.byref(p), ix.h, lam, K, fr, fqc, None, 0, C.byref(need)) == 0, L.smr_last_error(e.h)
        pinned = torch.empty(need.value + 64, dtype=torch.uint8, pin_memory=True)
        stages = {}

        def device():
            rep = open_report(outs["device"])
            rep.skip_pairwise()
            t0 = time.perf_counter()
            rc = L.smr_pairwise_part(e.h, 0, C.byref(p), ix.h, lam, K, fr, fqc, pinned.data_ptr(), pinned.numel(), C.byref(need))
            assert rc == 0, L.smr_last_error(e.h)
            t1 = time.perf_counter()
            rc = L.smr_report_add_pairwise(rep.h, 0, 0, pinned.data_ptr(), need.value)
            assert rc == 0, rc
            rep.close()
            stages["rows"], stages["write"] = (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

        for what, fn in [("(a) host: fetch + record_text + result_record + report_add per read", host), ("(b) device: pairwise_part (pinned) + report_add_pairwise", device)]:
            med, lo, hi = timed(fn, a.repeats)
            row = "  %-70s %9.1f ms [%.1f .. %.1f]  %6.1f M reads/s" % (what, med * 1e3, lo * 1e3, hi * 1e3, a.reads / med * 1e-6)
            if what.startswith("(b)"):
                row += "\n      last call: smr_pairwise_part %.1f ms wall (HIP events: %s), %d bytes out; smr_report_add_pairwise + close %.1f ms" % (
                    stages["rows"], ", ".join("%s %.1f ms" % kv for kv in e.pairwise_times().items()), need.value, stages["write"])
            lines.append(row)
            print(row, flush=True)
        names = ("aligned.blast",)
        same = all(open(os.path.join(outs["host"], f), "rb").read() == open(os.path.join(outs["device"], f), "rb").read() for f in names)
        assert same and sorted(os.listdir(outs["host"])) == sorted(os.listdir(outs["device"])), "the two paths wrote different files"
        lines.append("  files equal (aligned.blast %d bytes)" % tuple(os.path.getsize(os.path.join(outs["device"], f)) for f in names))
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
