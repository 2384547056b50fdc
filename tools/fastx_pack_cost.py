"""What parsing and packing a reads file costs on the device (smr_reads_upload_fastx_file) against the host's way (smr_reads_load_fastx_text
with a given number of threads + smr_reads_upload), on the same files: a FASTQ and a FASTA file of --reads reads of 150 nt (sortmerna_amd/synth.py
letters, fixed-width ids so that the files are written in one piece).  Per variant: wall time per call with the file in the page cache, after
one warm-up call, median of --repeats; for the device path the HIP-event times of its stages beside it.  Needs a GPU.

    python tools/fastx_pack_cost.py --reads 8000000 --threads 16 --out profiles/fastx_device_pack.log
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sortmerna_amd as smr  # noqa: E402
from sortmerna_amd import capi, synth  # noqa: E402


def write_files(d, n, read_len, seed):
    letters = synth.make_reads_fast(None, None, n, read_len=read_len, frac_db=0.0, seed=seed)
    ids = np.char.zfill(np.arange(n).astype("S8"), 8).view(np.uint8).reshape(n, 8)
    nl = np.full((n, 1), ord("\n"), dtype=np.uint8)
    fq, fa = os.path.join(d, "reads.fq"), os.path.join(d, "reads.fa")
    np.concatenate([np.full((n, 1), ord("@"), np.uint8), np.full((n, 1), ord("r"), np.uint8), ids, nl, letters, nl, np.full((n, 1), ord("+"), np.uint8), nl,
                    np.full((n, read_len), ord("I"), np.uint8), nl], axis=1).tofile(fq)
    np.concatenate([np.full((n, 1), ord(">"), np.uint8), np.full((n, 1), ord("r"), np.uint8), ids, nl, letters, nl], axis=1).tofile(fa)
    return fq, fa


def timed(fn, repeats):
    fn()                                                        # warm-up: page cache, buffers at their size, code objects loaded
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
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    e = smr.Engine(0)                                           # raises without a GPU
    L = capi.load()
    lines = ["fastx_pack_cost: %d reads of %d nt, host parser with %d threads (the machine shows %d cores), median of %d calls after one warm-up [min .. max]"
             % (a.reads, a.read_len, a.threads, os.cpu_count(), a.repeats)]
    with tempfile.TemporaryDirectory() as d:
        for path in write_files(d, a.reads, a.read_len, 1234):
            size = os.path.getsize(path)
            lines.append("%s: %d bytes, %.1f text bytes per read" % (os.path.basename(path), size, size / a.reads))
            digest = {}

            def host(keep=False):
                r = smr.Reads.from_fastx_text(path, a.threads)
                e.upload_reads(r, 1)
                if keep:
                    digest["host"] = r.digest
                r.free()

            def device(view, keep=False):
                def run():
                    r = e.upload_fastx(path, 1, view=view)
                    assert e.fastx_info()[0] == 0, "the host parser ran"
                    if keep:
                        digest["device"] = r.digest
                    r.free()
                return run

            def device_totals_only():
                err = C.create_string_buffer(256)
                assert L.smr_reads_upload_fastx_file(e.h, path.encode(), 1, 0, None, err, 256) == 0, err.value

            for what, fn in [("host: load_fastx_text(threads=%d) + upload" % a.threads, host), ("device, SMR_FASTX_VIEW", device(True)), ("device, words copied back", device(False)),
                             ("device, out = NULL", device_totals_only)]:
                med, lo, hi = timed(fn, a.repeats)
                row = "  %-44s %8.1f ms [%.1f .. %.1f]  %6.1f M reads/s  %5.2f GB/s of text" % (what, med * 1e3, lo * 1e3, hi * 1e3, a.reads / med * 1e-6, size / med * 1e-9)
                if what.startswith("device"):
                    row += "   stages (HIP events, last call): " + ", ".join("%s %.1f ms" % kv for kv in e.fastx_times().items())
                lines.append(row)
                print(row, flush=True)
            host(keep=True)                                     # (untimed: the digest walks every packed byte)
            device(False, keep=True)()
            assert digest["host"] == digest["device"], "the two paths packed different batches"
            lines.append("  digests equal")
    e.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
