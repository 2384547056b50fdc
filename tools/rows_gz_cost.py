"""What gzipped SAM / BLAST reports of a batch cost with the text deflated on the device (smr_rows_part_gz / smr_pairwise_part_gz into a pinned
buffer + smr_report_add_rows_gz / _add_pairwise_gz, close under zip_out) against the path before it (smr_rows_part / smr_pairwise_part +
smr_report_add_rows / _add_pairwise, the text deflated by zlib on one thread inside smr_report_close), on the same batch: the FASTQ file of
tools/rows_cost.py (--reads single-end reads of 150 nt, 10 % of them sampled from a synthetic database of --db-nt letters), uploaded once with
SMR_FASTX_KEEP | SMR_FASTX_VIEW, aligned and traced back once.  Once for SAM + BLAST tabular, once for BLAST pairwise.  Both paths write to
--dir (default /dev/shm).  Per path: wall time of the (index, part) call(s) plus smr_report_close after one warm-up call, median of --repeats,
the two shares apart for the last call; the bytes that cross the bus; for the device path the HIP-event times of the compressor; the size of
the files against zlib at levels 6 and 1 over the same bytes.  The two sets of files are compared after inflation in the same run.  Needs a GPU.

    python tools/rows_gz_cost.py --reads 8000000 --out profiles/rows_gz_cost.log
"""
import argparse
import ctypes as C
import gzip
import os
import shutil
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sortmerna_amd as smr  # noqa: E402
from sortmerna_amd import capi, report, synth  # noqa: E402
from fastx_split_cost import timed  # noqa: E402
from rows_cost import COLS, GUMBEL  # noqa: E402


def zsize(data, level):
    z = zlib.compressobj(level, zlib.DEFLATED, 31)
    return len(z.compress(data)) + len(z.flush())


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
    lines = ["rows_gz_cost: %d FASTQ reads of %d nt, single-end, 10 %% sampled from a synthetic database of %d nt, gzipped reports written to %s, wall time of "
             "the (index, part) call(s) + smr_report_close, median of %d after one warm-up [min .. max]" % (a.reads, a.read_len, a.db_nt, a.dir, a.repeats)]
    work = tempfile.mkdtemp(prefix="rows_gz_cost_", dir=a.dir)

    def say(row):
        lines.append(row)
        print(row, flush=True)

    try:
        db = os.path.join(work, "db.fasta")
        synth.make_db(db, a.db_nt, seed=42)
        codes, offs = synth.load_db_codes(db)
        fq = os.path.join(work, "reads.fq")
        synth.write_fastq(fq, synth.make_reads_fast(codes, offs, a.reads, read_len=a.read_len, frac_db=0.10, seed=1234, sub=0.005, indel=0.0001, n_rate=0.001))
        parts = smr.Index.build(db, 18, 3072.0, 10000, 0)
        assert len(parts) == 1
        ix = parts[0]
        reads = e.upload_fastx(fq, 1, view=True, keep=True)
        lam, K = GUMBEL
        p = smr.default_params(minimal_score=smr.minimal_score(lam, K, ix.info(), reads.count, reads.total_len))
        p.index_num, p.part, p.is_last_index_part = 0, 0, 1
        e.upload_index(ix, 0)
        e.align_part(0, p)
        e.traceback(0, p)
        fr, fqc = report.corrected_sizes(K, ix.info(), reads.count, reads.total_len)
        aligned = e.counters(1)["num_aligned"]
        say("reads.fq: %d bytes; %d of %d reads aligned (%.1f %%)" % (os.path.getsize(fq), aligned, a.reads, 100.0 * aligned / a.reads))
        o = capi.RowsOpts()
        o.want_sam, o.want_blast, o.blast_cols = 1, 1, " ".join(COLS).encode()
        o.lam, o.K, o.full_ref_corr, o.full_read_corr = lam, K, fr, fqc
        off, gz_off, need, plain = (C.c_uint64 * 3)(), (C.c_uint64 * 3)(), C.c_uint64(), C.c_uint64()
        pw = (e.h, 0, C.byref(p), ix.h, lam, K, fr, fqc)

        for what in ("SAM + BLAST tabular (%s)" % " ".join(COLS), "BLAST pairwise (-blast 0)"):
            pair = what.startswith("BLAST pairwise")
            names = ("aligned.blast",) if pair else ("aligned.sam", "aligned.blast")
            outs = {k: os.path.join(work, ("pair_" if pair else "rows_") + k) for k in ("host", "device")}
            for d in outs.values():
                os.makedirs(d)
            if pair:
                assert L.smr_pairwise_part(*pw, None, 0, C.byref(need)) == 0, L.smr_last_error(e.h)
            else:
                assert L.smr_rows_part(e.h, 0, C.byref(p), ix.h, C.byref(o), None, 0, off, C.byref(need)) == 0, L.smr_last_error(e.h)
            n_plain = need.value
            bound = e.gzip_lines_bound(n_plain, 1 if pair else 2)
            pinned = torch.empty(max(n_plain, bound) + 64, dtype=torch.uint8, pin_memory=True)
            stages = {}

            def open_report(d):
                rep = report.Report(d, True, fastx=False, other=False, blast_cols=None if pair else COLS, sam=not pair, blast_pairwise=pair, zip_out=True)
                rep.set_db(0, lam, K, fr, fqc)
                rep.set_part(0, 0, ix)
                return rep

            def host():                                        # the path before: the text crosses the bus, zlib deflates it at close
                rep = open_report(outs["host"])
                t0 = time.perf_counter()
                if pair:
                    assert L.smr_pairwise_part(*pw, pinned.data_ptr(), pinned.numel(), C.byref(need)) == 0, L.smr_last_error(e.h)
                    assert L.smr_report_add_pairwise(rep.h, 0, 0, pinned.data_ptr(), need.value) == 0
                else:
                    assert L.smr_rows_part(e.h, 0, C.byref(p), ix.h, C.byref(o), pinned.data_ptr(), pinned.numel(), off, C.byref(need)) == 0, L.smr_last_error(e.h)
                    assert L.smr_report_add_rows(rep.h, 0, 0, pinned.data_ptr(), off) == 0
                t1 = time.perf_counter()
                rep.close()
                stages["host"] = ((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, need.value)

            def device():                                      # the members cross the bus, close writes them as they are
                rep = open_report(outs["device"])
                t0 = time.perf_counter()
                if pair:
                    assert L.smr_pairwise_part_gz(*pw, pinned.data_ptr(), bound, C.byref(plain), C.byref(need)) == 0, L.smr_last_error(e.h)
                    assert L.smr_report_add_pairwise_gz(rep.h, 0, 0, pinned.data_ptr(), need.value) == 0
                else:
                    assert L.smr_rows_part_gz(e.h, 0, C.byref(p), ix.h, C.byref(o), pinned.data_ptr(), bound, gz_off, off, C.byref(need)) == 0, L.smr_last_error(e.h)
                    assert L.smr_report_add_rows_gz(rep.h, 0, 0, pinned.data_ptr(), gz_off) == 0
                t1 = time.perf_counter()
                rep.close()
                stages["device"] = ((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3, need.value)

            say("%s: %d plain bytes" % (what, n_plain))
            med = {}
            for key, label, fn in [("host", "(a) before: part call + report_add, zlib inside smr_report_close", host), ("device", "(b) device: part_gz call + report_add_gz, members written at close", device)]:
                med[key], lo, hi = timed(fn, a.repeats)
                call, close, crossed = stages[key]
                say("  %-70s %9.1f ms [%.1f .. %.1f]\n      last call: part call + add %.1f ms, smr_report_close %.1f ms; %d bytes crossed the bus" % (
                    label, med[key] * 1e3, lo * 1e3, hi * 1e3, call, close, crossed))
                if key == "device":
                    assert crossed <= bound, "need %d above smr_gzip_lines_bound %d" % (crossed, bound)
                    say("      compressor, HIP events: %s; the rows kernels: %s; %d bytes <= smr_gzip_lines_bound %d" % (
                        ", ".join("%s %.1f ms" % kv for kv in e.gzip_times().items()),
                        ", ".join("%s %.1f ms" % kv for kv in (e.pairwise_times() if pair else e.rows_times()).items()), crossed, bound))
            say("  (a) / (b) = %.1f" % (med["host"] / med["device"]))
            for f in names:
                text = gzip.open(os.path.join(outs["host"], f + ".gz"), "rb").read()
                assert gzip.open(os.path.join(outs["device"], f + ".gz"), "rb").read() == text, "%s: the two paths inflate to different files" % f
                sizes = [os.path.getsize(os.path.join(outs[k], f + ".gz")) for k in ("host", "device")]
                l6, l1 = zsize(text, 6), zsize(text, 1)
                say("  %s: %d bytes plain, equal after inflation; .gz before %d bytes, device %d bytes; zlib level 6 %d, level 1 %d; device / level 6 = %.2f, device / level 1 = %.2f" % (
                    f, len(text), sizes[0], sizes[1], l6, l1, sizes[1] / l6, sizes[1] / l1))
                del text
            assert sorted(os.listdir(outs["host"])) == sorted(os.listdir(outs["device"])), "the two paths wrote different files"
            for d in outs.values():
                shutil.rmtree(d, ignore_errors=True)
            del pinned
        reads.free()
    finally:
        shutil.rmtree(work, ignore_errors=True)
    e.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
