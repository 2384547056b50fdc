"""Known-answer vectors for the Smith-Waterman kernels at the ssw.h seam: seeded random (read, reference window) pairs run through
the reference's OWN ssw.c (oracle/_ref/libssw_ref.so = /root/reference/src/sortmerna/ssw.c compiled as it lies, oracle/Makefile),
called exactly like alignment.cpp:362-383 does: ssw_init(read, len, Read::initScoringMatrix's 5x5 matrix, 5, score_size 2) and
ssw_align(profile, ref, refLen, gap_open, gap_ext, flag 2, filters, 0, 0).

    python tests/golden/make_golden_ssw.py        # rewrites tests/golden/ssw_pairs.json
    python tests/golden/make_golden_ssw.py --sw16   # sw16_pairs.json: spans of 1..256 letters for k_sw16<13 | 19 | 26 | 32> (smr_sw16_batch)
    python tests/golden/make_golden_ssw.py --long   # ssw_pairs_long.json.gz: reads of 513 letters and more for the long-read strips (smr_ssw_batch mode 5)

Pairs: lengths 1..900 (a few up to 2500), ~1.5 % N in the read, reference window = a mutated copy of the read (substitutions,
insertions, deletions incl. long ones, N) inside random flanks, or an unrelated sequence; two scoring schemes."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
LIB = os.path.join(REPO, "oracle", "_ref", "libssw_ref.so")


class SAlign(C.Structure):      # include/ssw.h:58-71
    _fields_ = [("cigar", C.POINTER(C.c_uint32)), ("ref_num", C.c_uint32), ("ref_begin1", C.c_int32), ("ref_end1", C.c_int32),
                ("read_begin1", C.c_int32), ("read_end1", C.c_int32), ("readlen", C.c_uint32), ("score1", C.c_uint16), ("part", C.c_uint16),
                ("index_num", C.c_uint16), ("cigarLen", C.c_uint16), ("strand", C.c_bool)]


def ref_lib():
    L = C.CDLL(LIB)
    L.ssw_init.restype = C.c_void_p
    L.ssw_init.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int8]
    L.ssw_align.restype = C.POINTER(SAlign)
    L.ssw_align.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_uint8, C.c_uint8, C.c_uint8, C.c_uint16, C.c_int32, C.c_int32]
    L.init_destroy.argtypes = [C.POINTER(C.c_void_p)]
    L.align_destroy.argtypes = [C.POINTER(C.POINTER(SAlign))]
    return L


def scoring_matrix(match, mismatch, score_n):          # Read::initScoringMatrix, read.cpp:274-288
    m = []
    for a in range(4):
        m += [match if a == b else mismatch for b in range(4)] + [score_n]
    m += [score_n] * 5
    return np.array(m, dtype=np.int8)


def ssw_reference(L, read, ref, match, mismatch, score_n, go, ge, filters):
    """-> [score1, ref_begin1, ref_end1, read_begin1, read_end1] of the reference's ssw_align (flag 2)"""
    rd = np.frombuffer(read, dtype=np.int8).copy()
    rf = np.frombuffer(ref, dtype=np.int8).copy()
    mat = scoring_matrix(match, mismatch, score_n)
    prof = C.c_void_p(L.ssw_init(rd.ctypes.data, len(rd), mat.ctypes.data, 5, 2))
    a = L.ssw_align(prof, rf.ctypes.data, len(rf), go, ge, 2, filters, 0, 0)
    r = a.contents
    out = [int(r.score1), int(r.ref_begin1), int(r.ref_end1), int(r.read_begin1), int(r.read_end1)]
    L.align_destroy(C.byref(a))
    L.init_destroy(C.byref(prof))
    return out


def make_pairs(seed, n_pairs):
    rng = np.random.Generator(np.random.PCG64(seed))
    pairs = []
    for i in range(n_pairs):
        big = i % 40 == 39
        m = int(rng.integers(900, 2500)) if big else int(rng.integers(1, 900)) if i % 3 else int(rng.integers(18, 160))
        read = rng.integers(0, 4, size=m).astype(np.uint8)
        read[rng.random(m) < 0.015] = 4
        kind = i % 5
        if kind == 4:                                        # unrelated reference
            ref = rng.integers(0, 4, size=max(1, m + int(rng.integers(-10, 30)))).astype(np.uint8)
        else:
            sub = [0.01, 0.05, 0.12, 0.2][kind]
            out = []
            q = 0
            while q < m:
                u = rng.random()
                if u < sub:
                    out.append(int(rng.integers(0, 4))); q += 1
                elif u < sub + 0.01:
                    out.append(int(rng.integers(0, 4)))      # insertion in the reference
                elif u < sub + 0.02:
                    q += 1 if rng.random() < 0.7 else int(rng.integers(2, 12))      # deletion (sometimes long)
                elif u < sub + 0.025:
                    out.append(4); q += 1                    # N in the reference
                else:
                    out.append(int(read[q]) if read[q] < 4 else 0); q += 1
            fl, fr = int(rng.integers(0, 12)), int(rng.integers(0, 12))
            ref = np.array(list(rng.integers(0, 4, size=fl)) + out + list(rng.integers(0, 4, size=fr)), dtype=np.uint8)
            if ref.size == 0:
                ref = np.array([0], dtype=np.uint8)
        pairs.append((read.tobytes(), ref.tobytes()))
    return pairs


SCHEMES = [dict(match=2, mismatch=-3, score_N=-3, gap_open=5, gap_ext=2, filters=30), dict(match=5, mismatch=-4, score_N=-4, gap_open=5, gap_ext=2, filters=60)]


# Schemes under which ssw.c's striped kernels leave the affine recurrence (round 6: the library's slow path reproduces their stripe geometry,
# smr_sw_striped.hpp): gap_open <= gap_ext (the 16-bit kernel's early exit from its lazy-F loop, ssw.c:496-507), 2 * gap < |mismatch| (E stored
# before the lazy-F loop has raised H, ssw.c:267), a positive score for N.  -> ssw_pairs_striped.json (make_golden_ssw.py --striped)
STRIPED_SCHEMES = [dict(match=2, mismatch=-3, score_N=-3, gap_open=3, gap_ext=3, filters=30), dict(match=2, mismatch=-3, score_N=-3, gap_open=2, gap_ext=2, filters=30),
                   dict(match=2, mismatch=-5, score_N=-5, gap_open=2, gap_ext=1, filters=30), dict(match=1, mismatch=-3, score_N=-3, gap_open=1, gap_ext=1, filters=20),
                   dict(match=2, mismatch=-3, score_N=1, gap_open=5, gap_ext=2, filters=30), dict(match=2, mismatch=-3, score_N=-3, gap_open=5, gap_ext=2, filters=30)]


# ---- k_sw16 (smr_walk.hpp): spans of 1 .. 256 letters ---------------------------------------------------------------------------------
# The two predicates of the product, restated: a scheme the fast kernels take (scheme_unsupported, smr_engine.hip) and numbers that fit the
# packed 16-bit representation (sw_pk_fits, smr_sw_pk.hpp).  Every scheme and pair written to a file is asserted against both.
def scheme_unsupported(mismatch, score_N, gap_open, gap_ext):
    mm = max(-mismatch, -min(score_N, 0))
    return 2 * gap_open < mm or 2 * gap_ext < mm or score_N > 0 or gap_open <= gap_ext


def sw_pk_fits(m, n, match, mismatch, score_N, gap_open):
    return m * match + 255 < 32768 and n + 128 <= 8191 and gap_open + mismatch >= 0 and gap_open + score_N >= 0 and match + gap_open <= 255 and score_N + gap_open <= 255


SW16_ROWS = (13, 19, 26, 32)
# the two schemes of SCHEMES, then the corners of the two predicates: the largest match (256 x 127 + 255 = 32767) with match + gap_open = 255,
# gap_open + mismatch = 0, score_N = 0, gap_ext = 0 (which the first predicate allows only with mismatch = score_N = 0)
SW16_SCHEMES = SCHEMES + [dict(match=127, mismatch=-127, score_N=-127, gap_open=128, gap_ext=64, filters=1000),
                          dict(match=2, mismatch=-5, score_N=-5, gap_open=5, gap_ext=3, filters=30),
                          dict(match=2, mismatch=-3, score_N=0, gap_open=5, gap_ext=2, filters=30),
                          dict(match=2, mismatch=0, score_N=0, gap_open=1, gap_ext=0, filters=30)]


def sw16_lengths():
    ms = {1, 2, 3, 104, 105, 152, 153, 208, 209, 255, 256}
    for R in SW16_ROWS:
        ms |= {R - 1, R // 2}
        for k in range(1, 9):
            ms |= {x for x in (k * R - 1, k * R, k * R + 1) if 1 <= x <= min(8 * R, 256)}
    return sorted(ms)


def mutate(rng, read, sub, n_in_ref):
    out, q, m = [], 0, len(read)
    while q < m:
        u = rng.random()
        if u < sub:
            out.append(int(rng.integers(0, 4))); q += 1
        elif u < sub + 0.012:
            out.append(int(rng.integers(0, 4)))
        elif u < sub + 0.024:
            q += 1 if rng.random() < 0.7 else int(rng.integers(2, 9))
        elif n_in_ref and u < sub + 0.034:
            out.append(4); q += 1
        else:
            out.append(int(read[q]) if read[q] < 4 else 0); q += 1
    return out


def make_sw16_pairs(seed, lengths, shift=0):
    rng = np.random.Generator(np.random.PCG64(seed))
    pairs = []
    for i, m in enumerate(lengths):
        kind = (i + shift) % 8
        read = rng.integers(0, 4, size=m).astype(np.uint8)
        if kind in (0, 3, 5):                                   # N in the read (kinds 1, 2, 4, 6, 7: none)
            read[rng.random(m) < 0.03] = 4
        rnd = lambda k: list(rng.integers(0, 4, size=k))
        if kind in (0, 1):                                      # a mutated copy inside flanks: n up to about 2 m; kind 0 with N in the window
            fl, fr = int(rng.integers(0, m // 2 + 2)), int(rng.integers(0, m // 2 + 2))
            ref = rnd(fl) + mutate(rng, read, [0.02, 0.1][i // 8 % 2], kind == 0) + rnd(fr)
        elif kind == 2:                                         # unrelated, no N anywhere
            ref = rnd(max(1, m + int(rng.integers(-m // 2, m))))
        elif kind == 3:                                         # a window shorter than the read (a piece of it)
            a = int(rng.integers(0, max(1, m // 2))); b = a + max(1, int(rng.integers(1, max(2, m // 2))))
            ref = [int(x) if x < 4 else 0 for x in read[a:b]]
        elif kind == 4:                                         # the read matches the window at two offsets: equal scores, the earlier end column wins
            ref = rnd(int(rng.integers(0, 6))) + list(read) + rnd(int(rng.integers(0, 9))) + list(read) + rnd(int(rng.integers(0, 6)))
        elif kind == 5:                                         # one column
            ref = [int(rng.integers(0, 5))]
        elif kind == 6:                                         # a repeat against a repeat: every cell of a diagonal ties
            c = int(rng.integers(0, 4)); read[:] = c
            ref = [c] * max(1, m + int(rng.integers(-m // 3, m // 2 + 2)))
        else:                                                   # a two-letter repeat with one indel, N in the window only
            read = np.array([(q & 1) * 2 for q in range(m)], dtype=np.uint8)
            ref = [(q & 1) * 2 for q in range(m + 7)]
            ref.insert(len(ref) // 2, 1)
            if m > 4:
                ref[int(rng.integers(0, len(ref)))] = 4
        ref = np.array(ref[:600] if ref else [0], dtype=np.uint8)
        pairs.append((read.tobytes(), ref.tobytes()))
    return pairs


def write_cases(L, path, schemes_pairs, gz=False):
    out = {"alphabet": "ACGTN", "cases": []}
    tr = bytes.maketrans(bytes(range(5)), b"ACGTN")
    for sc, pairs in schemes_pairs:
        assert not scheme_unsupported(sc["mismatch"], sc["score_N"], sc["gap_open"], sc["gap_ext"]), sc
        for r, f in pairs:
            assert sw_pk_fits(len(r), len(f), sc["match"], sc["mismatch"], sc["score_N"], sc["gap_open"]), (sc, len(r), len(f))
        exp = [ssw_reference(L, r, f, sc["match"], sc["mismatch"], sc["score_N"], sc["gap_open"], sc["gap_ext"], sc["filters"]) for r, f in pairs]
        out["cases"].append(dict(scoring=sc, reads=[r.translate(tr).decode() for r, _ in pairs], refs=[f.translate(tr).decode() for _, f in pairs], expected=exp))
        print("scheme", sc, "pairs", len(pairs), "with begin", sum(1 for e in exp if e[1] >= 0), "max score", max(e[0] for e in exp))
    if gz:
        import gzip
        with gzip.GzipFile(path, "wb", mtime=0) as g:
            g.write(json.dumps(out).encode())
    else:
        json.dump(out, open(path, "w"))
    print(path, os.path.getsize(path), "bytes")


# ---- the long-read strips (sw_wave_long_r<8 ... 24>, smr_chain.hpp): reads of 513 letters up to what sw_pk_fits allows -------------------------
def sw_long_rows(m):                       # the cost model of smr_chain.hpp, restated only to CHOOSE lengths (the test asks the library which height a length selects)
    cost = lambda R: ((m + 128 * R - 1) // (128 * R)) * (14 * R + 35)
    best = 8
    for R in range(10, 25, 2):
        if cost(R) < cost(best):
            best = R
    return best


def long_lengths(match):
    top = (32768 - 255 - 1) // match
    by = {}
    for m in range(513, top + 1):
        by.setdefault(sw_long_rows(m), []).append(m)
    assert sorted(by) == list(range(8, 25, 2)), sorted(by)
    ms = set()
    for R, v in by.items():
        full = [m for m in v if m % (128 * R) == 0]           # the last strip is full
        one = [m for m in v if m % (128 * R) == 1]            # ... holds one row
        ms |= {v[0], v[-1], v[len(v) // 2]} | set(full[:1]) | set(one[:1])
    return sorted(ms | {513, top})


def make_long_pairs(seed, lengths):
    rng = np.random.Generator(np.random.PCG64(seed))
    pairs = []
    for i, m in enumerate(lengths):
        read = rng.integers(0, 4, size=m).astype(np.uint8)
        read[rng.random(m) < 0.01] = 4
        # the window: a mutated copy of a PIECE of the read (cost is m x n) with indels of up to tens of letters, N in it; every fourth the whole read
        whole = i % 4 == 3 and m <= 4000                       # (smr_ssw_batch holds read + 9 x window in 60 KB of LDS)
        a = 0 if whole else int(rng.integers(0, m - 400))
        b = m if whole else min(m, a + int(rng.integers(300, 900)))
        out, q = [], a
        while q < b:
            u = rng.random()
            if u < 0.04:
                out.append(int(rng.integers(0, 4))); q += 1
            elif u < 0.045:
                out += list(rng.integers(0, 4, size=int(rng.integers(1, 40))))
            elif u < 0.05:
                q += int(rng.integers(1, 40))
            elif u < 0.056:
                out.append(4); q += 1
            else:
                out.append(int(read[q]) if read[q] < 4 else 0); q += 1
        ref = np.array(list(rng.integers(0, 4, size=int(rng.integers(0, 20)))) + out + list(rng.integers(0, 4, size=int(rng.integers(0, 20)))), dtype=np.uint8)
        pairs.append((read.tobytes(), ref.tobytes()))
    return pairs


def main():
    if "--sw16" in sys.argv or "--long" in sys.argv:
        assert os.path.isfile(LIB), "make -C oracle ref"
        L = ref_lib()
        if "--sw16" in sys.argv:
            ms = sw16_lengths()
            sp = [(sc, make_sw16_pairs(20261016 + k, ms if k < 2 else ms[k % 2::2], 3 * k)) for k, sc in enumerate(SW16_SCHEMES)]
            write_cases(L, os.path.join(HERE, "sw16_pairs.json"), sp)
        else:
            sp = [(sc, make_long_pairs(20261116 + k, long_lengths(sc["match"]))) for k, sc in enumerate(SCHEMES)]
            write_cases(L, os.path.join(HERE, "ssw_pairs_long.json.gz"), sp, gz=True)
        return 0
    assert os.path.isfile(LIB), "make -C oracle ref  (needs /root/reference)"
    L = ref_lib()
    out = {"alphabet": "ACGTN", "cases": []}
    if "--striped" in sys.argv:
        for k, sc in enumerate(STRIPED_SCHEMES):
            pairs = make_pairs(20261001 + k, 100)
            exp = [ssw_reference(L, r, f, sc["match"], sc["mismatch"], sc["score_N"], sc["gap_open"], sc["gap_ext"], sc["filters"]) for r, f in pairs]
            tr = bytes.maketrans(bytes(range(5)), b"ACGTN")
            out["cases"].append(dict(scoring=sc, reads=[r.translate(tr).decode() for r, _ in pairs], refs=[f.translate(tr).decode() for _, f in pairs], expected=exp))
            print("scheme", sc, "pairs", len(pairs), "with begin", sum(1 for e in exp if e[1] >= 0), "max score", max(e[0] for e in exp))
        json.dump(out, open(os.path.join(HERE, "ssw_pairs_striped.json"), "w"))
        print(os.path.getsize(os.path.join(HERE, "ssw_pairs_striped.json")), "bytes")
        return 0
    for k, sc in enumerate(SCHEMES):
        pairs = make_pairs(20260926 + k, 160)
        exp = [ssw_reference(L, r, f, sc["match"], sc["mismatch"], sc["score_N"], sc["gap_open"], sc["gap_ext"], sc["filters"]) for r, f in pairs]
        tr = bytes.maketrans(bytes(range(5)), b"ACGTN")
        out["cases"].append(dict(scoring=sc, reads=[r.translate(tr).decode() for r, _ in pairs], refs=[f.translate(tr).decode() for _, f in pairs], expected=exp))
        print("scheme", k, "pairs", len(pairs), "with begin", sum(1 for e in exp if e[1] >= 0), "max score", max(e[0] for e in exp))
    json.dump(out, open(os.path.join(HERE, "ssw_pairs.json"), "w"))
    print(os.path.getsize(os.path.join(HERE, "ssw_pairs.json")), "bytes")


if __name__ == "__main__":
    sys.exit(main())
