"""Known-answer vectors that sit ON the limits of the traceback kernels (tests/golden/make_golden_trace.py draws at random and does not):
constructed (read, reference window) pairs run through the reference's OWN ssw.c (oracle/_ref/libssw_ref.so), ssw_align(..., flag 2,
filters 1), which returns banded_sw's CIGAR with the alignment.  Stored per pair: its name, both sequences, score1 / begin / end positions
and the CIGAR operations; one case per (class, scoring scheme).

    python tests/golden/make_golden_trace_limits.py        # rewrites tests/golden/trace_limits.json.gz

Gaps are runs of N (code 4) in the read or the reference: a random filler gets aligned through and smears the path, N never does -- every
stored path is the clean gap that was meant (checked below: the CIGAR of every gap / shift / edge pair has exactly the runs it was built
for).  Flanks are random ACGT, each worth more than the gap next to it costs, so that the local alignment keeps both sides.

  gap    one gap of d letters between two flanks, as I and as D: initial band d + 1, on both sides of every hand-over of the ladder
         (3|4, 7|8, 31|32, 255|256, 2047|2048) and of the strip counts 1|2 (band 31|32) and 2|3 (band 63|64)
  shift  equal spans: an insertion of d N, a flank, a deletion of d N (and the mirror image): the band starts at 1 and doubles, the
         pair is handed from kernel to kernel with its band parked
  edge   the path on the outermost diagonal of a band that is not doubled: "hi" (deletion of bw, flank, insertion of 1) reaches
         diagonal 2 bw, "lo" (insertion of bw, flank, deletion of 2 bw - 1) reaches diagonal 0
  runs   blocks of 12 letters with alternating 1-letter insertions and deletions between them: 2 k + 1 runs inside band 1, around the
         24 runs that are staged per alignment; with one more gap of 3 (7) letters the same in the 16-lane (the wide) kernel
  tiny   prefixes / suffixes of 1..7 and 1..11 letters of one random sequence (S0).  ssw.c's begin / end positions cut every one of
         them to the common k letters: the spans that reach the kernels are 1 x 1 .. 7 x 7, all kM.  Spans that really differ come
         from the same N gap between flanks of 1..3 letters (S1, S2; gaps of 1..4 as I and as D): windows shorter and longer than
         the read within 11 letters, bands wider than the window
  fill   the gap class with a filler of random ACGT letters instead of N, 62..256 letters, around the strip boundaries: ssw.c
         aligns into the filler, H next to the gap comes from the diagonal as well as from E / F, and the "gap opened" bits of the
         flags -- which an N gap never consults -- decide the walk where two strips meet
  big    a 2 100-, a 1 900- and a 1 300-letter read against a copy with 2 % substitutions.  The longest read of a batch sizes the LDS
         of the narrow kernels (32 bytes of flags per row and 8 x 2 windows: they fit up to about 1 340 letters): the first two
         switch them off for the batch that holds them, the third leaves them on with 63 of the 64 KB taken

The table this prints (per case: initial band |refSpan - readSpan| + 1, largest deviation |j - i| of the stored path from the main
diagonal, run count) is what the conditions at the end are checked on."""
import gzip
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_ssw as G  # noqa: E402
from make_golden_trace import ssw_with_cigar  # noqa: E402

S0 = dict(match=2, mismatch=-3, score_N=-3, gap_open=5, gap_ext=2, filters=1)
S1 = dict(match=5, mismatch=-4, score_N=-4, gap_open=5, gap_ext=1, filters=1)
S2 = dict(match=5, mismatch=-4, score_N=-4, gap_open=1, gap_ext=2, filters=1)      # gap_open < gap_ext: the F scan has to iterate
SCHEMES = {"S0": S0, "S1": S1, "S2": S2}

GAP_D = (1, 2, 3, 6, 7, 30, 31, 62, 63, 64, 254, 255, 2046, 2047)
SHIFT_D = (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 128, 129, 256, 257)
EDGE_BW = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 33, 63, 64, 65, 127, 128)
RUNS_K = range(9, 16)


def N(n):
    return np.full(n, 4, dtype=np.uint8)


def cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts]).tobytes()


def gap_cost(sc, d):
    return sc["gap_open"] + (d - 1) * sc["gap_ext"]


def flank(sc, d):
    """letters per flank next to a gap of d: max(40, d / 4 + 40), and more where the scheme makes that gap dearer than such a flank scores"""
    return max(40, d // 4 + 40, gap_cost(sc, d) // sc["match"] + 8)


def gap_pairs(rng, sc, ds):
    out = []
    for d in ds:
        fl = flank(sc, d)
        for kind in "ID":
            a, b = rng.integers(0, 4, fl), rng.integers(0, 4, fl)
            lng, sht = cat(a, N(d), b), cat(a, b)
            out.append(("gap%d%s" % (d, kind), lng if kind == "I" else sht, sht if kind == "I" else lng, 3))
    return out


def shift_pairs(rng, sc, ds):
    out = []
    for d in ds:
        fl = flank(sc, d)
        a, b, c = rng.integers(0, 4, fl), rng.integers(0, 4, fl), rng.integers(0, 4, fl)
        x, y = cat(a, N(d), b, c), cat(a, b, N(d), c)
        out.append(("shift%dID" % d, x, y, 5))
        out.append(("shift%dDI" % d, y, x, 5))
    return out


def edge_pairs(rng, sc, bws):
    out = []
    for bw in bws:
        fl = flank(sc, 2 * bw - 1)
        a, b, c = rng.integers(0, 4, fl), rng.integers(0, 4, fl), rng.integers(0, 4, fl)
        out.append(("hi%d" % bw, cat(a, b, N(1), c), cat(a, N(bw), b, c), 5))
        out.append(("lo%d" % bw, cat(a, N(bw), b, c), cat(a, b, N(2 * bw - 1), c), 5))
    return out


def runs_pairs(rng, sc):
    """k indels of one letter, alternately in the read and in the reference; extra: one more gap of N in the reference behind the first block"""
    out = []
    for extra in (0, 3, 7):
        for k in RUNS_K:
            for odd in (0, 1):
                rd, rf = [], []
                for q in range(k):
                    blk = list(rng.integers(0, 4, 12))
                    rd += blk; rf += blk
                    if q == 0 and extra:
                        blk = list(rng.integers(0, 4, 12))
                        rf += [4] * extra; rd += blk; rf += blk
                    (rd if (q + (1 if extra else 0)) % 2 == 0 else rf).append(int(rng.integers(0, 4)))      # (behind the extra gap: away from the main diagonal first)
                blk = list(rng.integers(0, 4, 12 + odd))
                out.append(("runs%d_%d%s" % (k, odd, "+%d" % extra if extra else ""), cat(rd + blk), cat(rf + blk), 2 * k + 1 + (2 if extra else 0)))
    return out


def runs24_pair(rng):
    """under S2 a substitution is cheaper as 1I1D (1 + 1) than as a mismatch (4): ten indels and one substitution inside a block are 24 runs"""
    rd, rf = [], []
    for q in range(10):
        blk = list(rng.integers(0, 4, 12))
        rd += blk; rf += blk
        (rd if q % 2 == 0 else rf).append(int(rng.integers(0, 4)))
        if q == 4:
            rd[-7] = (rd[-7] + 1) % 4
    blk = list(rng.integers(0, 4, 12))
    return [("runs24", cat(rd + blk), cat(rf + blk), None)]


def tiny_pairs(rng):
    out = []
    for m in range(1, 8):
        for n in range(1, 12):
            a = rng.integers(0, 4, max(m, n))
            out.append(("pre%d_%d" % (m, n), cat(a[:m]), cat(a[:n]), None))
            out.append(("suf%d_%d" % (m, n), cat(a[a.size - m:]), cat(a[a.size - n:]), None))
    return out


def tiny_gap_pairs(rng):
    out = []
    for fa in (1, 2, 3):
        for fb in (1, 2, 3):
            for g in (1, 2, 3, 4):
                a, b = rng.integers(0, 4, fa), rng.integers(0, 4, fb)
                out.append(("gap%d_%d_%dI" % (fa, g, fb), cat(a, N(g), b), cat(a, b), None))
                out.append(("gap%d_%d_%dD" % (fa, g, fb), cat(a, b), cat(a, N(g), b), None))
    return out


FILL_D = (62, 63, 64, 65, 126, 127, 128, 129, 254, 255, 256)


def fill_pairs(rng, sc, ds):
    out = []
    for d in ds:
        fl = flank(sc, d)
        for kind in "ID":
            a, b, x = rng.integers(0, 4, fl), rng.integers(0, 4, fl), rng.integers(0, 4, d)
            lng, sht = cat(a, x, b), cat(a, b)
            out.append(("fill%d%s" % (d, kind), lng if kind == "I" else sht, sht if kind == "I" else lng, None))
    return out


def big_pairs(rng):
    out = []
    for m in (2100, 1900, 1300):
        a = rng.integers(0, 4, m)
        b = a.copy()
        hit = rng.random(m) < 0.02
        b[hit] = (b[hit] + 1 + rng.integers(0, 3, int(hit.sum()))) % 4
        out.append(("big%d" % m, cat(a), cat(b), None))
    return out


def path_stats(cig):
    """largest |j - i| along the path of a CIGAR that starts on the main diagonal, and its run count"""
    i = j = dev = 0
    for x in cig:
        n, op = x >> 4, x & 15
        if op != 2:
            i += n
        if op != 1:
            j += n
        dev = max(dev, abs(j - i))
    return dev, len(cig)


def build_cases():
    cases = []       # (class, scheme name, [(name, read, ref, runs the pair was built for | None)])
    seed = 0
    for cls, names, make in (("gap", ("S1", "S2"), gap_pairs), ("shift", ("S1", "S2"), shift_pairs), ("edge", ("S1", "S2"), edge_pairs)):
        for s in names:
            seed += 1
            rng = np.random.Generator(np.random.PCG64(4100 + seed))
            arg = {"gap": [d for d in GAP_D if s == "S1" or d <= 255], "shift": SHIFT_D, "edge": EDGE_BW}[cls]
            cases.append((cls, s, make(rng, SCHEMES[s], arg)))
    for k, s in enumerate(("S0", "S1")):
        cases.append(("runs", s, runs_pairs(np.random.Generator(np.random.PCG64(4200 + k)), SCHEMES[s])))
    cases.append(("runs", "S2", runs24_pair(np.random.Generator(np.random.PCG64(4210)))))
    cases.append(("tiny", "S0", tiny_pairs(np.random.Generator(np.random.PCG64(4300)))))
    for k, s in enumerate(("S1", "S2")):
        cases.append(("tiny", s, tiny_gap_pairs(np.random.Generator(np.random.PCG64(4310 + k)))))
    for k, s in enumerate(("S1", "S2")):
        cases.append(("fill", s, fill_pairs(np.random.Generator(np.random.PCG64(4500 + k)), SCHEMES[s], FILL_D)))
    for k, s in enumerate(("S0", "S1", "S2")):
        cases.append(("big", s, big_pairs(np.random.Generator(np.random.PCG64(4400 + k)))))
    return cases


def compact(v):
    v = sorted(set(v))
    return ",".join(map(str, v)) if len(v) <= 34 else "%d..%d (%d values)" % (v[0], v[-1], len(v))


def main():
    assert os.path.isfile(G.LIB), "make -C oracle ref  (needs the reference's sources)"
    L = G.ref_lib()
    tr = bytes.maketrans(bytes(range(5)), b"ACGTN")
    out = {"alphabet": "ACGTN", "cases": []}
    per_kernel = {}      # kernel of the runs pairs (by initial band) -> run counts
    tiny_spans = set()   # (read span, reference span, initial band) of the tiny class
    for cls, s, pairs in build_cases():
        sc = SCHEMES[s]
        names, reads, refs, exp, cigs, band0, devs, runs = [], [], [], [], [], [], [], []
        dropped = 0
        for name, r, f, built_for in pairs:
            e, cg = ssw_with_cigar(L, r, f, sc)
            if cg is None:
                dropped += 1
                continue
            dev, n = path_stats(cg)
            b0 = abs((e[2] - e[1]) - (e[4] - e[3])) + 1
            assert built_for is None or n == built_for, "%s %s %s: %d runs, built for %d" % (cls, s, name, n, built_for)
            names.append(name); reads.append(r.translate(tr).decode()); refs.append(f.translate(tr).decode()); exp.append(e); cigs.append(cg)
            band0.append(b0); devs.append(dev); runs.append(n)
            if cls == "tiny":
                tiny_spans.add((e[4] - e[3] + 1, e[2] - e[1] + 1, b0))
            if cls == "runs":
                assert dev <= b0, name                       # the initial band holds the path: the kernel that starts is the one that finishes
                per_kernel.setdefault("band<8>" if b0 <= 3 else "band<16>" if b0 <= 7 else "wide", []).append(n)
        assert cls != "tiny" or s != "S0" or dropped == 0
        out["cases"].append(dict(kind=cls, scheme=s, scoring=sc, names=names, reads=reads, refs=refs, expected=exp, cigars=cigs))
        print("%-5s %s pairs %3d dropped %d | initial band %s | deviation %s | runs %s" % (cls, s, len(names), dropped, compact(band0), compact(devs), compact(runs)))
        # what the class is there for
        if cls == "gap":
            assert sorted(set(band0)) == [d + 1 for d in GAP_D if s == "S1" or d <= 255] and band0 == [d + 1 for d in devs]
        if cls == "shift":
            assert set(band0) == {1} and sorted(set(devs)) == list(SHIFT_D)
        if cls == "edge":
            for name, b0, dev, cg in zip(names, band0, devs, cigs):
                bw = int(name[2:])
                assert b0 == bw and dev == bw and (cg[1] & 15) == (2 if name.startswith("hi") else 1), name      # diagonal 2 bw | 0 of the band as it starts
    assert max(max(m, n) for m, n, _ in tiny_spans) <= 11 and (1, 1, 1) in tiny_spans
    shorter = sorted((m, n) for m, n, _ in tiny_spans if n < m)
    longer = sorted((m, n) for m, n, _ in tiny_spans if n > m)
    beyond = sorted((m, n, b) for m, n, b in tiny_spans if 2 * b + 1 > n and b > 1)
    assert shorter and longer and beyond and min(n for m, n in shorter) == 2
    print("tiny spans (read x window): window shorter %s | longer %s | band wider than the window %d shapes" % (
        " ".join("%dx%d" % x for x in shorter), " ".join("%dx%d" % x for x in longer), len(beyond)))
    for kern in ("band<8>", "band<16>", "wide"):
        v = per_kernel[kern]
        assert any(21 <= n <= 24 for n in v) and any(25 <= n <= 28 for n in v), (kern, v)
        print("runs in %-8s %s" % (kern, compact(v)))
    print("a pair of exactly 24 runs: %s" % ("stored" if any(24 in v for v in per_kernel.values()) else "none (ssw.c produced none)"))
    path = os.path.join(HERE, "trace_limits.json.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as f:
        f.write(json.dumps(out, separators=(",", ":")).encode())
    print(os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < os.path.getsize(os.path.join(HERE, "trace_pairs.json.gz"))


if __name__ == "__main__":
    sys.exit(main())
