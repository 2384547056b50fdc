"""What writing the reports of mates in two reads files costs on the device (smr_rows_part_mates / smr_pairwise_part_mates into a pinned buffer +
smr_report_add_rows / _add_pairwise) against the host's way (smr_results_fetch of both batches, then per pair smr_reads_record_text,
smr_result_record_batch and smr_report_add_pair: the loop of examples/smr_align.cpp under --mates host, run in native code by
tools/mates_host_loop.cpp), on the same two batches: --pairs pairs of FASTQ reads of 150 nt in two files, 10 % of the reads sampled from the
synthetic database of tools/rows_cost.py, uploaded once into batches 0 and 1 with SMR_FASTX_KEEP | SMR_FASTX_VIEW, aligned and traced back
once.  Once for SAM + BLAST tabular, once for BLAST pairwise; then the same under zip_out: the _gz forms against zlib inside
smr_report_close.  Every path writes to --dir (default /dev/shm).  Per path: wall time per call after one warm-up call, median of --repeats;
for the device path the split of smr_mates_times and the `write` times of the plain calls' kernels beside it.  The files of the two paths
are compared in the same run.  The baseline is path (a) of the same run.  Needs a GPU and g++.

    python tools/mates_rows_cost.py --pairs 4000000 --out profiles/mates_rows_cost.log
"""
import argparse
import ctypes as C
import gzip
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sortmerna_amd as smr  # noqa: E402
from sortmerna_amd import build, capi, report, synth  # noqa: E402
from fastx_split_cost import timed  # noqa: E402
from rows_cost import COLS, GUMBEL  # noqa: E402


def host_loop_library(d):
    so = os.path.join(d, "libmates_host_loop.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", os.path.join(ROOT, "tools", "mates_host_loop.cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", build.LIBDIR, "-lsmr_hip", "-Wl,-rpath," + build.LIBDIR, "-o", so])
    lib = C.CDLL(so)
    lib.mates_host_loop.restype = C.c_int
    lib.mates_host_loop.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--db-nt", type=int, default=2000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch                                                # (the pinned buffer)
    e = smr.Engine(0)                                           # raises without a GPU
    L = capi.load()
    lines = []

    def say(row):
        lines.append(row)
        print(row, flush=True)

    say("mates_rows_cost: %d pairs of FASTQ reads of %d nt in two files (batches 0 and 1), 10 %% sampled from a synthetic database of %d nt, reports written to %s, "
        "median of %d calls after one warm-up [min .. max]" % (a.pairs, a.read_len, a.db_nt, a.dir, a.repeats))
    work = tempfile.mkdtemp(prefix="mates_cost_", dir=a.dir)
    code = tempfile.mkdtemp(prefix="mates_cost_")              # (a memory file system is often mounted noexec)
    try:
        host_lib = host_loop_library(code)
        db = os.path.join(work, "db.fasta")
        synth.make_db(db, a.db_nt, seed=42)
        codes, offs = synth.load_db_codes(db)
        parts = smr.Index.build(db, 18, 3072.0, 10000, 0)
        assert len(parts) == 1
        ix = parts[0]
        e.upload_index(ix, 0)
        reads = []
        for k in (0, 1):
            fq = os.path.join(work, "reads_%d.fq" % (k + 1))
            synth.write_fastq(fq, synth.make_reads_fast(codes, offs, a.pairs, read_len=a.read_len, frac_db=0.10, seed=1234 + k, sub=0.005, indel=0.0001, n_rate=0.001))
            e.select_batch(k)
            reads.append(e.upload_fastx(fq, 1, view=True, keep=True))
            os.remove(fq)
        n_all, len_all = sum(r.count for r in reads), sum(r.total_len for r in reads)
        lam, K = GUMBEL
        p = smr.default_params(minimal_score=smr.minimal_score(lam, K, ix.info(), n_all, len_all))
        p.index_num, p.part, p.is_last_index_part = 0, 0, 1
        aligned = 0
        for k in (0, 1):
            e.select_batch(k)
            e.align_part(0, p)
            e.traceback(0, p)
            aligned += e.counters(1)["num_aligned"]
        e.select_batch(0)
        fr, fqc = report.corrected_sizes(K, ix.info(), n_all, len_all)
        say("%d of %d reads aligned (%.1f %%)" % (aligned, n_all, 100.0 * aligned / n_all))
        o = capi.RowsOpts()
        o.want_sam, o.want_blast, o.blast_cols = 1, 1, " ".join(COLS).encode()
        o.lam, o.K, o.full_ref_corr, o.full_read_corr = lam, K, fr, fqc
        off, gz_off, need, plain = (C.c_uint64 * 3)(), (C.c_uint64 * 3)(), C.c_uint64(), C.c_uint64()
        rw = (e.h, 1, 0, C.byref(p), ix.h, C.byref(o))
        pw = (e.h, 1, 0, C.byref(p), ix.h, lam, K, fr, fqc)

        for pair in (False, True):
            what = "BLAST pairwise (-blast 0)" if pair else "SAM + BLAST tabular (%s)" % " ".join(COLS)
            names = ("aligned.blast",) if pair else ("aligned.sam", "aligned.blast")
            if pair:
                assert L.smr_pairwise_part_mates(*pw, None, 0, C.byref(need)) == 0, L.smr_last_error(e.h)
            else:
                assert L.smr_rows_part_mates(*rw, None, 0, off, C.byref(need)) == 0, L.smr_last_error(e.h)
            n_plain = need.value
            bound = e.gzip_lines_bound(n_plain, 1 if pair else 2)
            pinned = torch.empty(max(n_plain, bound) + 64, dtype=torch.uint8, pin_memory=True)
            # the write kernels of the two batches as the plain calls time them (the same kernels on the same batches)
            plain_write = 0.0
            for k in (0, 1):
                e.select_batch(k)
                if pair:
                    assert L.smr_pairwise_part(e.h, 0, C.byref(p), ix.h, lam, K, fr, fqc, pinned.data_ptr(), pinned.numel(), C.byref(need)) == 0, L.smr_last_error(e.h)
                    plain_write += e.pairwise_times()["write"]
                else:
                    assert L.smr_rows_part(e.h, 0, C.byref(p), ix.h, C.byref(o), pinned.data_ptr(), pinned.numel(), off, C.byref(need)) == 0, L.smr_last_error(e.h)
                    plain_write += e.rows_times()["write"]
            e.select_batch(0)
            for zipped in (False, True):
                outs = {k: os.path.join(work, "%s%s_%s" % ("pair" if pair else "rows", "_gz" if zipped else "", k)) for k in ("host", "device")}
                for d in outs.values():
                    os.makedirs(d)
                stages = {}

                def open_report(d):
                    rep = report.Report(d, True, fastx=False, other=False, blast_cols=None if pair else COLS, sam=not pair, blast_pairwise=pair, zip_out=zipped)
                    rep.set_db(0, lam, K, fr, fqc)
                    rep.set_part(0, 0, ix)
                    return rep

                def host():
                    rep = open_report(outs["host"])
                    t0 = time.perf_counter()
                    rc = host_lib.mates_host_loop(e.h, reads[0].h, reads[1].h, rep.h, 1)
                    assert rc == 0, rc
                    t1 = time.perf_counter()
                    rep.close()
                    stages["host"] = ((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3)

                def device():
                    rep = open_report(outs["device"])
                    t0 = time.perf_counter()
                    if pair and zipped:
                        assert L.smr_pairwise_part_mates_gz(*pw, pinned.data_ptr(), bound, C.byref(plain), C.byref(need)) == 0, L.smr_last_error(e.h)
                        assert L.smr_report_add_pairwise_gz(rep.h, 0, 0, pinned.data_ptr(), need.value) == 0
                    elif pair:
                        assert L.smr_pairwise_part_mates(*pw, pinned.data_ptr(), pinned.numel(), C.byref(need)) == 0, L.smr_last_error(e.h)
                        assert L.smr_report_add_pairwise(rep.h, 0, 0, pinned.data_ptr(), need.value) == 0
                    elif zipped:
                        assert L.smr_rows_part_mates_gz(*rw, pinned.data_ptr(), bound, gz_off, off, C.byref(need)) == 0, L.smr_last_error(e.h)
                        assert L.smr_report_add_rows_gz(rep.h, 0, 0, pinned.data_ptr(), gz_off) == 0
                    else:
                        assert L.smr_rows_part_mates(*rw, pinned.data_ptr(), pinned.numel(), off, C.byref(need)) == 0, L.smr_last_error(e.h)
                        assert L.smr_report_add_rows(rep.h, 0, 0, pinned.data_ptr(), off) == 0
                    t1 = time.perf_counter()
                    rep.close()
                    stages["device"] = ((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3)

                say("%s%s: %d plain bytes" % (what, ", zip_out" if zipped else "", n_plain))
                med = {}
                labels = {"host": "(a) host: fetch + record_text + result_record + report_add_pair per pair" + (", zlib inside smr_report_close" if zipped else ""),
                          "device": "(b) device: %s_part_mates%s (pinned) + report_add%s" % ("pairwise" if pair else "rows", "_gz" if zipped else "", "_gz" if zipped else "")}
                for key, fn in (("host", host), ("device", device)):
                    med[key], lo, hi = timed(fn, a.repeats)
                    say("  %-90s %9.1f ms [%.1f .. %.1f]  %6.1f M pairs/s\n      last call: loop / part call + add %.1f ms, smr_report_close %.1f ms" % (
                        labels[key], med[key] * 1e3, lo * 1e3, hi * 1e3, a.pairs / med[key] * 1e-6, stages[key][0], stages[key][1]))
                t = e.mates_times()
                say("      smr_mates_times, HIP events: %s; %d bytes crossed the bus" % (", ".join("%s %.1f ms" % kv for kv in t.items()), need.value))
                if zipped:
                    say("      compressor, HIP events: %s" % ", ".join("%s %.1f ms" % kv for kv in e.gzip_times().items()))
                rate = n_plain / (t["interleave"] * 1e-3) * 1e-9 if t["interleave"] > 0 else 0.0
                say("      interleave %.2f ms (%.1f GB/s of output; read and written once each) against %.2f ms for the write kernels of the two batches in the plain calls%s" % (
                    t["interleave"], rate, plain_write, ": the interleave takes LONGER than the two write kernels together" if t["interleave"] > plain_write else ""))
                say("  (a) / (b) = %.1f" % (med["host"] / med["device"]))
                for f in names:
                    fn_ = f + (".gz" if zipped else "")
                    rd = (lambda path: gzip.open(path, "rb").read()) if zipped else (lambda path: open(path, "rb").read())
                    assert rd(os.path.join(outs["host"], fn_)) == rd(os.path.join(outs["device"], fn_)), "%s: the two paths wrote different files" % fn_
                assert sorted(os.listdir(outs["host"])) == sorted(os.listdir(outs["device"])), "the two paths wrote different files"
                say("  files equal%s (%s)" % (" after inflation" if zipped else "", ", ".join("%s %d bytes" % (f + (".gz" if zipped else ""), os.path.getsize(os.path.join(outs["device"], f + (".gz" if zipped else "")))) for f in names)))
                for d in outs.values():
                    shutil.rmtree(d, ignore_errors=True)
            del pinned
        for r in reads:
            r.free()
    finally:
        shutil.rmtree(work, ignore_errors=True)
        shutil.rmtree(code, ignore_errors=True)
    e.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
