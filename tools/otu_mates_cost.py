"""What writing otu_map.txt and aligned_denovo.fq of mates in two reads files (-otu_map -de_novo_otu, thresholds 0.97 / 0.97) costs on the device
(smr_otu_part_mates and smr_fastx_denovo of layout 2 into pinned buffers + smr_report_add_otu + smr_report_add_denovo) against the host's way
(smr_results_fetch of both batches, then per pair smr_reads_record_text, smr_result_record_batch and smr_report_add_pair: the loop of
examples/smr_align.cpp under --otu-mates host, run in native code by tools/mates_host_loop.cpp on a report opened with the OTU switches), on the
same two batches: the workload of tools/mates_rows_cost.py -- --pairs pairs of FASTQ reads of 150 nt in two files, 10 % of the reads sampled
from a synthetic database of --db-nt letters --, uploaded once into batches 0 and 1 with SMR_FASTX_KEEP | SMR_FASTX_VIEW, aligned, traced back
and passed through smr_idcov_part once each.  --hot samples those 10 % from the FIRST reference only, so that nearly every member of the map
falls into one group.  Both paths write to --dir (default /dev/shm).  Per path: wall time per call after one warm-up call, median of
--repeats; for the device path the HIP-event times of smr_otu_times and smr_otu_mates_times beside it.  The two sets of files are compared in
the same run.  The baseline is path (a) of the same run.  Needs a GPU and g++.

    python tools/otu_mates_cost.py --pairs 4000000 --out profiles/otu_mates_cost.log
    python tools/otu_mates_cost.py --pairs 4000000 --hot --out profiles/otu_mates_cost.log --append
"""
import argparse
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import sortmerna_amd as smr  # noqa: E402
from sortmerna_amd import capi, report, synth  # noqa: E402
from fastx_split_cost import timed  # noqa: E402
from mates_rows_cost import host_loop_library  # noqa: E402
from rows_cost import GUMBEL  # noqa: E402

MIN_ID = MIN_COV = 0.97


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--db-nt", type=int, default=2000000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hot", action="store_true", help="every read that comes from the database comes from its first reference")
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="write behind what --out holds (the --hot run behind the even one)")
    a = ap.parse_args()
    import torch                                                # (the pinned buffers)
    e = smr.Engine(0)                                           # raises without a GPU
    L = capi.load()
    lines = []

    def say(row):
        lines.append(row)
        print(row, flush=True)

    say("otu_mates_cost%s: %d pairs of FASTQ reads of %d nt in two files (batches 0 and 1), 10 %% sampled from %s a synthetic database of %d nt, -otu_map -de_novo_otu at "
        "%.2f / %.2f written to %s, median of %d calls after one warm-up [min .. max]" % (" --hot" if a.hot else "", a.pairs, a.read_len, "the first reference of" if a.hot else "",
                                                                                          a.db_nt, MIN_ID, MIN_COV, a.dir, a.repeats))
    work = tempfile.mkdtemp(prefix="otu_mates_cost_", dir=a.dir)
    code = tempfile.mkdtemp(prefix="otu_mates_cost_")          # (a memory file system is often mounted noexec)
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
            synth.write_fastq(fq, synth.make_reads_fast(codes, offs[:2] if a.hot else offs, a.pairs, read_len=a.read_len, frac_db=0.10, seed=1234 + k, sub=0.005, indel=0.0001,
                                                        n_rate=0.001))
            e.select_batch(k)
            reads.append(e.upload_fastx(fq, 1, view=True, keep=True))
            os.remove(fq)
        n_all, len_all = sum(r.count for r in reads), sum(r.total_len for r in reads)
        lam, K = GUMBEL
        p = smr.default_params(minimal_score=smr.minimal_score(lam, K, ix.info(), n_all, len_all))
        p.index_num, p.part, p.is_last_index_part = 0, 0, 1
        aligned, ic = 0, {}
        for k in (0, 1):
            e.select_batch(k)
            e.align_part(0, p)
            e.traceback(0, p)
            e.idcov_part(0, p, MIN_ID, MIN_COV)
            aligned += e.counters(1)["num_aligned"]
            for key, v in e.idcov_counters().items():
                ic[key] = ic.get(key, 0) + v
        e.select_batch(0)
        say("%d of %d reads aligned (%.1f %%); the pass over both batches: %s" % (aligned, n_all, 100.0 * aligned / n_all, ", ".join("%s %d" % kv for kv in ic.items())))
        outs = {k: os.path.join(work, k) for k in ("host", "device")}
        for d in outs.values():
            os.makedirs(d)

        def open_report(d):
            rep = report.Report(d, True, fastx=False, other=False, otu_map=True, denovo=True, min_id=MIN_ID, min_cov=MIN_COV)
            rep.set_part(0, 0, ix)
            return rep

        def host():
            rep = open_report(outs["host"])
            rc = host_lib.mates_host_loop(e.h, reads[0].h, reads[1].h, rep.h, 1)
            assert rc == 0, rc
            rep.close()

        need, any_ = (C.c_uint64 * 2)(), C.c_int()
        args = (e.h, 1, 0, C.byref(p), ix.h, MIN_ID, MIN_COV)
        assert L.smr_otu_part_mates(*args, None, 0, None, 0, need, C.byref(any_)) == 0, L.smr_last_error(e.h)
        pinned = torch.empty(need[0] + 64, dtype=torch.uint8, pin_memory=True)
        gpinned = torch.empty((need[1] + 1) * 16, dtype=torch.uint8, pin_memory=True)      # (the table of groups as well: a pageable destination makes the copy wait for the host)
        groups = gpinned.numpy().view(smr.engine.OTU_GROUP)
        o = capi.FxSplitOpts(2, 0, 0, 0, 0, 1, 0)               # layout 2: the mates in batch 1
        doff, dneed = (C.c_uint64 * 5)(), C.c_uint64()
        assert L.smr_fastx_denovo(e.h, 1, C.byref(o), None, None, 0, doff, C.byref(dneed)) == 0, L.smr_last_error(e.h)
        dpinned = torch.empty(dneed.value + 64, dtype=torch.uint8, pin_memory=True)
        stages = {"otu": [], "denovo": [], "write": []}

        def device():
            rep = open_report(outs["device"])
            rep.skip_otu()
            rep.skip_denovo()
            t0 = time.perf_counter()
            rc = L.smr_otu_part_mates(*args, pinned.data_ptr(), pinned.numel(), groups.ctypes.data, len(groups), need, C.byref(any_))
            assert rc == 0, L.smr_last_error(e.h)
            t1 = time.perf_counter()
            rc = L.smr_fastx_denovo(e.h, 1, C.byref(o), None, dpinned.data_ptr(), dpinned.numel(), doff, C.byref(dneed))
            assert rc == 0, L.smr_last_error(e.h)
            t2 = time.perf_counter()
            assert L.smr_report_add_otu(rep.h, 0, 0, pinned.data_ptr(), need[0], groups.ctypes.data, need[1], any_.value) == 0
            assert L.smr_report_add_denovo(rep.h, dpinned.data_ptr(), doff) == 0
            rep.close()
            for k, v in zip(("otu", "denovo", "write"), ((t1 - t0) * 1e3, (t2 - t1) * 1e3, (time.perf_counter() - t2) * 1e3)):
                stages[k].append(v)

        med = {}
        for key, what, fn in [("host", "(a) host: fetch + record_text + result_record + report_add_pair per pair", host),
                              ("device", "(b) device: otu_part_mates + fastx_denovo layout 2 (pinned) + report_add_otu + report_add_denovo", device)]:
            med[key], lo, hi = timed(fn, a.repeats)
            say("  %-100s %9.1f ms [%.1f .. %.1f]  %6.1f M pairs/s" % (what, med[key] * 1e3, lo * 1e3, hi * 1e3, a.pairs / med[key] * 1e-6))
        big = int(groups["n_reads"][:need[1]].max()) if need[1] else 0
        med_of = {k: (float(np.median(v[1:])), min(v[1:]), max(v[1:])) for k, v in stages.items()}          # (without the warm-up call)
        say("      wall time inside, median [min .. max]: smr_otu_part_mates %.1f ms [%.1f .. %.1f], %d members in %d groups, the largest %d, %d bytes out; "
            "smr_fastx_denovo %.1f ms [%.1f .. %.1f], %d bytes out; smr_report_add_otu + smr_report_add_denovo + close %.1f ms [%.1f .. %.1f]" % (
                med_of["otu"] + (int(groups["n_reads"][:need[1]].sum()), need[1], big, need[0]) + med_of["denovo"] + (dneed.value,) + med_of["write"]))
        t, tm = e.otu_times(), e.otu_mates_times()
        say("      smr_otu_times of the last call, HIP events: %s" % ", ".join("%s %.2f ms" % kv for kv in t.items()))
        say("      smr_otu_mates_times of the last call, HIP events: %s" % ", ".join("%s %.2f ms" % kv for kv in tm.items()))
        two = tm["classify_a"] + tm["sizes_a"] + tm["classify_b"] + tm["sizes_b"]
        say("      the merged compaction %.2f ms against %.2f ms for the two classify and size stages%s" % (
            tm["compact"], two, ": the compaction takes LONGER than the two stages together" if tm["compact"] > two else ""))
        say("  (a) / (b) = %.1f" % (med["host"] / med["device"]))
        names = sorted(os.listdir(outs["host"]))
        assert names == sorted(os.listdir(outs["device"])) and "otu_map.txt" in names and "aligned_denovo.fq" in names, names
        same = all(open(os.path.join(outs["host"], f), "rb").read() == open(os.path.join(outs["device"], f), "rb").read() for f in names)
        assert same, "the two paths wrote different files"
        say("  files equal (%s)" % ", ".join("%s %d bytes" % (f, os.path.getsize(os.path.join(outs["device"], f))) for f in names))
        for r in reads:
            r.free()
    finally:
        shutil.rmtree(work, ignore_errors=True)
        shutil.rmtree(code, ignore_errors=True)
    e.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
