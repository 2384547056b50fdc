"""What inflating a gzip reads file costs on the device (smr_reads_upload_fastx_file under SMR_FASTX_INFLATE: the DEFLATE decoder kernels of
csrc/smr_gunzip.hpp, the compressed bytes cross the bus and the text never does) against the host's way (the same call without the flag: zlib
on the calling thread, then the H2D of the text), on the same file: FASTQ reads of 150 nt gzipped at level 6, in the page cache.  The file is
compressed the way pigz does it -- pieces of 32 MB deflated by a pool of processes, each closed with a full flush, laid end to end as one
member -- because one zlib stream over 2.5 GB would take minutes to make; zlib's blocks are what they would be.  The file is made before the
engine is, so no process but this one ever has the GPU open.  Per path: wall time per call
after one warm-up call, median of the repeats, with out == NULL (only the totals come back) and with a SMR_FASTX_VIEW object (the text is
copied back once); the HIP-event times of smr_gunzip_times and smr_fastx_times beside the device path.  Then smr_gunzip_batch, sizes only --
the whole decoder, no copy back -- for several values of `grain`.  The bundled amplicon file is measured the same way.  Needs a GPU.

    python tools/gunzip_cost.py --reads 8000000 --out profiles/gunzip_cost.log
"""
import argparse
import ctypes as C
import multiprocessing
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sortmerna_amd as smr  # noqa: E402
from sortmerna_amd import engine as eng  # noqa: E402
from fastx_pack_cost import write_files  # noqa: E402

AMPLICON = os.path.join(ROOT, "tests", "golden", "config2", "set2_environmental_study_550_amplicon.fasta.gz")
PIECE = 32 << 20


def _deflate_piece(job):
    path, at, n, last = job
    with open(path, "rb") as f:
        f.seek(at)
        data = f.read(n)
    z = zlib.compressobj(6, zlib.DEFLATED, -15)
    return z.compress(data) + (z.flush() if last else z.flush(zlib.Z_FULL_FLUSH)), zlib.crc32(data), len(data)


def gzip_file(src, dst, procs):
    size = os.path.getsize(src)
    jobs = [(src, at, min(PIECE, size - at), at + PIECE >= size) for at in range(0, size, PIECE)]
    crc = 0
    # (fresh interpreters, started before this process opens the GPU -- main() makes the file first --, and fewer than 16 of them)
    with multiprocessing.get_context("spawn").Pool(min(procs, 15)) as pool, open(dst, "wb") as g:
        g.write(b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff")
        for raw, c, n in pool.imap(_deflate_piece, jobs):
            g.write(raw)
            crc = _crc_combine(crc, c, n)
        g.write(int(crc).to_bytes(4, "little") + (size & 0xFFFFFFFF).to_bytes(4, "little"))
    return os.path.getsize(dst)


def _crc_combine(crc1, crc2, len2):
    """zlib's crc32_combine, which Python's zlib does not export: crc1 through len2 zero bytes (GF(2) matrix squaring), then ^ crc2"""
    if len2 == 0:
        return crc1

    def times(mat, vec):
        s, i = 0, 0
        while vec:
            if vec & 1:
                s ^= mat[i]
            vec >>= 1
            i += 1
        return s

    def square(mat):
        return [times(mat, mat[n]) for n in range(32)]

    odd = [0xEDB88320] + [1 << n for n in range(31)]
    even = square(odd)
    odd = square(even)
    while True:
        even = square(odd)
        if len2 & 1:
            crc1 = times(even, crc1)
        len2 >>= 1
        if not len2:
            break
        odd = square(even)
        if len2 & 1:
            crc1 = times(odd, crc1)
        len2 >>= 1
        if not len2:
            break
    return crc1 ^ crc2


def timed(fn, repeats):
    fn()                                                        # warm-up: page cache, buffers at their size, code objects loaded
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def measure(e, lines, what, path, n_reads, a):
    L = e.L
    gz = os.path.getsize(path)

    def say(row):
        lines.append(row)
        print(row, flush=True)

    def upload(flags, view):
        def fn():
            h = C.c_void_p()
            err = C.create_string_buffer(512)
            rc = L.smr_reads_upload_fastx_file(e.h, path.encode(), 1, flags | (eng.FASTX_VIEW if view else 0), C.byref(h) if view else None, err, 512)
            assert rc == 0, err.value
            if view:
                L.smr_reads_free(h)
        return fn

    say("%s: %d bytes of gzip%s" % (what, gz, ", %d reads" % n_reads if n_reads else ""))
    plain = None
    for view in (False, True):
        for name, flags, rp in (("host: zlib on the calling thread, then the text H2D", 0, a.host_repeats), ("device: SMR_FASTX_INFLATE", eng.FASTX_INFLATE, a.repeats)):
            med, lo, hi = timed(upload(flags, view), rp)
            info = e.fastx_info()
            assert info[0] == 0, "the host parser ran"
            plain = info[3]
            row = "  %-58s %-22s %10.1f ms [%.1f .. %.1f]  %7.1f MB/s of text (median of %d)" % (name, "SMR_FASTX_VIEW object" if view else "out == NULL", med * 1e3, lo * 1e3, hi * 1e3, plain / med * 1e-6, rp)
            if flags:
                g = e.gunzip_info()
                assert g["path"] == "device", g
                row += "\n      last call: gunzip %s; %s\n      HIP events: gunzip %s; parse and pack %s" % (
                    ", ".join("%s %s" % (k, g[k]) for k in ("candidates", "tasks", "rounds", "members", "stored", "fixed", "dynamic")), "%d -> %d bytes" % (g["compressed"], g["plain"]),
                    ", ".join("%s %.2f" % kv for kv in e.gunzip_times().items()), ", ".join("%s %.2f" % kv for kv in e.fastx_times().items()))
            say(row)
    say("  (%d bytes of text)" % plain)
    blob = np.fromfile(path, dtype=np.uint8)
    need = C.c_uint64()
    for grain in a.grains:
        def fn():
            assert L.smr_gunzip_batch(e.h, blob.ctypes.data, blob.size, grain, None, 0, C.byref(need)) == 0
        med, lo, hi = timed(fn, a.repeats)
        g = e.gunzip_info()
        say("  smr_gunzip_batch, sizes only, grain %-8s %10.1f ms [%.1f .. %.1f]  %7.1f MB/s of text; %s, %d tasks, %d rounds; HIP events: %s" % (
            grain or "default", med * 1e3, lo * 1e3, hi * 1e3, need.value / med * 1e-6, g["path"], g["tasks"], g["rounds"], ", ".join("%s %.2f" % kv for kv in e.gunzip_times().items())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=8000000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--grains", type=lambda s: [int(x) for x in s.split(",")], default=[0, 1, 65536, 262144])
    ap.add_argument("--procs", type=int, default=15, help="processes that compress the file (15 at the most)")
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["gunzip_cost: smr_reads_upload_fastx_file of a gzip file with and without SMR_FASTX_INFLATE, wall time per call after one warm-up [min .. max], files in %s" % a.dir]
    work = tempfile.mkdtemp(prefix="gunz_cost_", dir=a.dir)
    try:
        fq, fa = write_files(work, a.reads, a.read_len, 1234)
        os.remove(fa)
        gz = fq + ".gz"
        t0 = time.perf_counter()
        gzip_file(fq, gz, a.procs)
        print("compressed in %.1f s" % (time.perf_counter() - t0), flush=True)
        os.remove(fq)
        e = smr.Engine(0)                                       # raises without a GPU; only now: the pool above is gone
        measure(e, lines, "FASTQ reads of %d nt, level 6" % a.read_len, gz, a.reads, a)
        os.remove(gz)
        measure(e, lines, "the amplicon file (tests/golden/config2)", AMPLICON, 0, a)
        e.close()
    finally:
        shutil.rmtree(work, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
