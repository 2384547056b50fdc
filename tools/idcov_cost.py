"""What the %id / %coverage pass (smr_idcov_part) costs next to the traceback of the same batch and next to the host loop over the same alignments.

    python tools/idcov_cost.py --workload illumina150            # bench.py's default workload: one batch of 8 M reads against the 140 Mnt DB
    python tools/idcov_cost.py --workload pacbio5k               # 50 000 reads of ~5 kb against the 14 Mnt DB

The workload is bench.py's (same DB files, same seeded batch 0).  Prints one JSON line: min / median / max over --rounds rounds of k_trace and
k_idcov milliseconds (HIP events on the engine's stream, smr_prof_kernels) and of the wall time of the smr_idcov_part call (collect +
read-back + the kernels), the alignments walked, the four totals, and what the host loop of smr_report.cpp needs for the same alignments
on one thread (host_walk_ms_one_thread; how it is taken is said where it is done)."""
import argparse
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["illumina150", "pacbio5k"], default="illumina150")
    ap.add_argument("--batch-reads", type=int, default=0)
    ap.add_argument("--db-nt", type=int, default=0)
    ap.add_argument("--min-id", type=float, default=0.97)
    ap.add_argument("--min-cov", type=float, default=0.97)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    import sortmerna_amd as smr
    from sortmerna_amd import synth
    args = argparse.Namespace(workload=a.workload, read_len=150, long_read_len=5000,
                              db_nt=a.db_nt or (14_000_000 if a.workload == "pacbio5k" else 140_000_000),
                              batch_reads=a.batch_reads or bench.WORKLOADS[a.workload]["batch_reads"])
    cache = os.path.join(tempfile.gettempdir(), "smr_bench_%s_%d" % (args.workload, args.db_nt))
    os.makedirs(cache, exist_ok=True)
    dbs = [p for _, p in bench.workload_dbs(args, synth, cache, 0)]
    codes, offs = bench.load_all_codes(synth, dbs)
    eng = smr.Engine(0)
    parts = smr.Index.build_gpu(eng, dbs[0], 18, 3072.0, 10000)
    slots = list(range(len(parts)))
    for s, ix in zip(slots, parts):
        eng.upload_index(ix, s)
    import ctypes as C
    import statistics
    from sortmerna_amd import report
    blob, o = bench.make_batch(args, synth, codes, offs, args.batch_reads, 1234)
    h = C.c_void_p()
    assert smr.capi.load().smr_reads_pack(blob, o.ctypes.data, len(o) - 1, C.byref(h)) == 0
    reads = smr.Reads(h)
    eng.upload_reads(reads, 1)
    p = smr.default_params(minimal_score=smr.minimal_score(bench.GUMBEL[0], bench.GUMBEL[1], parts[0].info(), reads.count, reads.total_len))
    out = dict(workload=a.workload, reads=reads.count, nt_per_read=reads.total_len / max(reads.count, 1), min_id=a.min_id, min_cov=a.min_cov, rounds=a.rounds)
    tr, ki, wl = [], [], []
    for rep in range(a.rounds + 1):                          # the first round is dropped (allocations, first launches)
        eng.reset_state()
        eng.prof_reset()
        smr.align_resident(eng, slots, [p], with_cigar=True)
        t0 = time.perf_counter()
        for part, s in enumerate(slots):
            p.index_num, p.part = 0, part
            eng.idcov_part(s, p, a.min_id, a.min_cov)
        wall = (time.perf_counter() - t0) * 1e3
        if rep:
            tr.append(eng.prof().trace_ms); ki.append(eng.prof_kernels()["k_idcov"]["ms"]); wl.append(wall)
    tot = eng.idcov_counters()
    stat = lambda v: dict(min=min(v), median=statistics.median(v), max=max(v))
    out.update(trace_ms=stat(tr), k_idcov_ms=stat(ki), idcov_part_wall_ms=stat(wl), alignments=sum(tot.values()), totals=tot, num_aligned=eng.counters(1)["num_aligned"])
    # The host loop that walks the same letters today: smr_report.cpp (Read::calc_miss_gap_match for the BLAST rows; the otu_map writer has the
    # same loop).  Records of a pass with thresholds 0 -- every alignment passes, so the map writer walks every one of them -- go through
    # smr_report_add twice on one host thread: with no output selected (record parse + call overhead) and with otu_map (the same + the walk
    # + one map entry per alignment).  The difference is the walk.
    eng.reset_state()
    smr.align_resident(eng, slots, [p], with_cigar=True)
    for part, s in enumerate(slots):
        p.index_num, p.part = 0, part
        eng.idcov_part(s, p, 0.0, 0.0)
    eng.fetch()
    hit = [(i, eng.record(i)) for i in range(reads.count) if eng.is_hit(i)]
    hit = [(">r%d" % i, blob[int(o[i]):int(o[i + 1])].decode(), r) for i, r in hit if r]
    host = {}
    for name, kw in (("parse_only", {}), ("otu_map", dict(otu_map=True))):
        ts = []
        for rep in range(3):
            d = tempfile.mkdtemp(prefix="idcov_cost_")
            rp = report.Report(d, is_fastq=False, fastx=False, other=False, **kw)
            for k, ix in enumerate(parts):
                rp.set_part(0, k, ix)
            t0 = time.perf_counter()
            for hdr, seq, rec in hit:
                rp.add(hdr, seq, None, rec)
            ts.append((time.perf_counter() - t0) * 1e3)
            rp.close()
        host[name] = stat(ts)
    out.update(host_alignments=len(hit), host_add_ms=host, host_walk_ms_one_thread=host["otu_map"]["min"] - host["parse_only"]["min"])
    print(json.dumps(out))
    eng.close()


if __name__ == "__main__":
    main()
