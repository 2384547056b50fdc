"""The prefix tasks of k_sw16<13 | 19 | 26 | 32> (smr_walk.hpp, SW16_PREFIX) through smr_sw16_prefix_batch: the interval [lo, hi] that the first
`cols` columns of a window give for the score of the whole window, against a plain DP written here, over pairs of tests/golden/sw16_pairs.json
(whose full scores are ssw.c's) and pairs drawn here.  The same bodies run on the GPU (tests/test_gpu_sw16_prefix.py) and on the wave64
emulator (tests/test_emu_sw16_prefix.py).  Every check counts the tasks it compared and returns that number.  TEST INFRASTRUCTURE."""
import numpy as np

import sortmerna_amd as smr
from . import sw16

ROWS = sw16.ROWS
SCHEMES = sw16.SCHEMES


_H = {}


def matrix(span, win, sc):
    """H of the textbook affine-gap recurrence as an (m, n) array, one anti-diagonal at a time (a cell needs the two diagonals before its own);
    column j depends on no column right of it, so H[:, :cols] is the matrix of the prefix.  Kept per (span, window, scheme): the tests ask for
    several cols, both strands and four instantiations of the same pairs"""
    key = (bytes(span), bytes(win), sc["match"], sc["mismatch"], sc["score_N"], sc["gap_open"], sc["gap_ext"])
    if key in _H:
        return _H[key]
    a = np.frombuffer(bytes(span), dtype=np.uint8).astype(np.int64)
    b = np.frombuffer(bytes(win), dtype=np.uint8).astype(np.int64)
    m, n = a.size, b.size
    S = np.where(a[:, None] == b[None, :], sc["match"], sc["mismatch"]).astype(np.int64)
    S[a == 4, :] = sc["score_N"]
    S[:, b == 4] = sc["score_N"]
    low = -(1 << 40)
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    E = np.full((m + 1, n + 1), low, dtype=np.int64)
    F = np.full((m + 1, n + 1), low, dtype=np.int64)
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        E[i, j] = np.maximum(E[i, j - 1] - sc["gap_ext"], H[i, j - 1] - sc["gap_open"])
        F[i, j] = np.maximum(F[i - 1, j] - sc["gap_ext"], H[i - 1, j] - sc["gap_open"])
        H[i, j] = np.maximum(np.maximum(H[i - 1, j - 1] + S[i - 1, j - 1], 0), np.maximum(E[i, j], F[i, j]))
    _H[key] = H[1:, 1:]
    return _H[key]


def row_maxima(span, win, cols, sc):
    """M_i, i < m: the maximum of H over row i of the first `cols` columns"""
    return [int(x) for x in matrix(span, win, sc)[:, :cols].max(axis=1)]


def interval(span, win, cols, sc):
    """[lo, hi] as include/smr_hip.h states them, from the DP's row maxima"""
    m, rem = len(span), len(win) - cols
    M = row_maxima(span, win, cols, sc)
    s = max(sc["match"], sc["mismatch"], sc["score_N"], 0)
    lo = max(M)
    hi = max([lo, s * min(m, rem)] + [M[i] + s * min(m - 1 - i, rem) for i in range(m)])
    return [lo, hi]


def cols_of(nref):
    """4, 8 and the largest multiple of 4 below nref, where they are below nref"""
    return sorted({c for c in (4, 8, (nref - 1) // 4 * 4) if 0 < c < nref})


class PrefixList(sw16.TaskList):
    """a TaskList whose tasks are (read, aq, m, reversed, win_off, nref, cols); expected = [lo, hi]; full = the score of the whole window or None"""

    def __init__(self, seed):
        super().__init__(seed)
        self.full = []

    def add_prefix(self, span, window, cols, sc, reversed_, pre=0, post=0, full=None, what="", read=None, off=None):
        r, aq = read if read is not None else self.add_read(span, reversed_, pre, post)
        off = off if off is not None else self.add_window(window, int(self.rng.integers(0, 5)))
        for c in cols:
            self.tasks.append((r, aq, len(span), reversed_, off, len(window), c))
            self.expected.append(interval(span, window, c, sc))
            self.full.append(full)
            self.what.append("%s, cols %d" % (what, c))
        return (r, aq), off

    def shuffle(self):
        o = self.rng.permutation(len(self.tasks))
        for name in ("tasks", "expected", "what", "full"):
            setattr(self, name, [getattr(self, name)[i] for i in o])

    def check(self, engine, rows, sc, blocks=0, force_any_n=False, label=""):
        rd = smr.Reads.from_seqs(self.reads)
        try:
            engine.upload_reads(rd, 1)
            got = engine.sw16_prefix_batch(self.tasks, bytes(self.ref), rows, blocks=blocks, force_any_n=force_any_n, **sw16._sc(sc))
        finally:
            rd.free()
        assert got.shape == (len(self.tasks), 2)
        for i, t in enumerate(self.tasks):
            where = "k_sw16<%d> prefix %s scoring %s blocks %d: task %d of %d (%s; m %d, reversed %d, window %d, cols %d)" % (rows, label, sc, blocks, i, len(self.tasks), self.what[i], t[2], t[3], t[5], t[6])
            assert got[i].tolist() == self.expected[i], "%s: got %s, the DP's row maxima give %s" % (where, got[i].tolist(), self.expected[i])
            if self.full[i] is not None:
                assert got[i][0] <= self.full[i] <= got[i][1], "%s: the whole window scores %d, outside %s" % (where, self.full[i], got[i].tolist())
        return len(self.tasks)


def fixture_pairs(rows, every=1):
    out = []
    for ci, c in enumerate(sw16.load()):
        idx = [i for i in range(len(c["reads_b"])) if len(c["reads_b"][i]) <= 8 * rows and len(c["refs_b"][i]) >= 5][::every]
        out.append((ci, c, idx))
    return out


def fixture_size(rows, every=1):
    return sum(2 * len(cols_of(len(c["refs_b"][i]))) for _, c, idx in fixture_pairs(rows, every) for i in idx)


def check_fixture(engine, rows, every=1):
    """the stored pairs (windows of at least five letters) on both strands with cols = 4, 8 and the largest multiple of 4 below the window: lo and hi
    are the DP's, and ssw.c's score of the whole window lies between them"""
    n = 0
    for ci, c, idx in fixture_pairs(rows, every):
        tl = PrefixList(7000 + 10 * rows + ci)
        for k, i in enumerate(idx):
            for rev in (0, 1):
                pre, post = (0, 0) if k % 2 == 0 else (int(tl.rng.integers(0, 70)), int(tl.rng.integers(0, 70)))
                tl.add_prefix(c["reads_b"][i], c["refs_b"][i], cols_of(len(c["refs_b"][i])), c["scoring"], rev, pre, post, full=c["expected"][i][0], what="pair %d of scheme %d" % (i, ci))
        tl.shuffle()
        n += tl.check(engine, rows, c["scoring"], label="fixture")
    return n


def _shapes(rows):
    top = min(8 * rows, 256)
    ms = sorted({1, 7, 8, 9, top - 1, top})
    return [(m, n) for m in ms for n in sorted({5, 8, 9, m + 8})]


def n_shapes(rows):
    return sum(len(cols_of(n)) for _, n in _shapes(rows))


def check_shapes(engine, rows, sc, seed=11):
    """m in {1, 7, 8, 9, 8 rows - 1, 8 rows} x nref in {5, 8, 9, m + 8} x every cols of cols_of, both strands and windows with and without N by turns;
    the whole window's score from the plain DP of helpers/swdp.py"""
    tl = PrefixList(seed * 100 + rows)
    for k, (m, n) in enumerate(_shapes(rows)):
        span, win = sw16._draw(tl.rng, m, n, k % 2, n_read=k % 3 == 0, n_win=k % 4 == 1)
        tl.add_prefix(span, win, cols_of(n), sc, k % 2, pre=k % 5, post=(k * 7) % 11, full=sw16._dp(span, win, sc)[0], what="shape %d x %d" % (m, n))
    tl.shuffle()
    n = tl.check(engine, rows, sc, label="shapes")
    assert n == n_shapes(rows)
    return n


N_QUADS = 16 * 16


def check_quads_and_cols(engine, rows, sc, seed=12):
    """sixteen waves: the problem under test in each quad position in turn with one cols, its neighbours other problems with cols that differ from quad to
    quad (the wave runs to its longest prefix: a short prefix next to a long one meets the columns past its own)"""
    tl = PrefixList(seed * 100 + rows)
    rng = tl.rng
    top = min(8 * rows, 256)
    span, win = sw16._draw(rng, top - 3, top + 30, 0)
    full = sw16._dp(span, win, sc)[0]
    rd0 = tl.add_read(span, 1, 7, 9)
    off0 = tl.add_window(win)
    pool = []
    for k in range(10):
        s, w = sw16._draw(rng, int(rng.integers(1, top + 1)), int(rng.integers(9, 300)), k % 2, n_win=k % 3 == 0)
        pool.append((s, w, k % 2, tl.add_read(s, k % 2, int(rng.integers(0, 30)), int(rng.integers(0, 30))), tl.add_window(w, 2), sw16._dp(s, w, sc)[0]))
    cache = {}
    for wave in range(16):
        for pos in range(16):
            if pos == wave:
                tl.add_prefix(span, win, [4 * (1 + wave * (((len(win) - 1) // 4 - 1) // 15))], sc, 1, full=full, what="the problem under test at quad %d" % pos, read=rd0, off=off0)
            else:
                k = int(rng.integers(0, len(pool)))
                s, w, rev, rd, off, f = pool[k]
                c = 4 * int(rng.integers(1, (len(w) - 1) // 4 + 1))
                if (k, c) not in cache:
                    cache[(k, c)] = interval(s, w, c, sc)
                tl.tasks.append((rd[0], rd[1], len(s), rev, off, len(w), c)); tl.expected.append(cache[(k, c)]); tl.full.append(f); tl.what.append("neighbour, cols %d" % c)
    assert len(tl.tasks) == N_QUADS
    return tl.check(engine, rows, sc, label="quads")


LIST_SIZES = (1, 15, 16, 17)
N_LISTS = sum(LIST_SIZES)


def check_list_sizes(engine, rows, sc, seed=13):
    """lists of 1, 15, 16 and 17 prefix tasks (a partial last pass; lists A and B empty)"""
    base = PrefixList(seed * 100 + rows)
    rng = base.rng
    top = min(8 * rows, 256)
    pool = []
    for k in range(6):
        s, w = sw16._draw(rng, int(rng.integers(1, top + 1)), int(rng.integers(9, 200)), k % 2, n_win=k % 3 == 0)
        c = 4 * int(rng.integers(1, (len(w) - 1) // 4 + 1))
        pool.append((base.add_read(s, k % 2, 3, 5), len(s), k % 2, base.add_window(w, 1), len(w), c, interval(s, w, c, sc), sw16._dp(s, w, sc)[0]))
    n = 0
    for size in LIST_SIZES:
        tl = PrefixList(0)
        tl.reads, tl.ref = base.reads, base.ref
        for q in range(size):
            rd, m, rev, off, nref, c, exp, f = pool[int(rng.integers(0, len(pool)))]
            tl.tasks.append((rd[0], rd[1], m, rev, off, nref, c)); tl.expected.append(exp); tl.full.append(f); tl.what.append("list of %d" % size)
        n += tl.check(engine, rows, sc, blocks=2 if size == 17 else 0, label="list of %d" % size)
    return n


def check_refusals(engine):
    """cols = 0, cols not a multiple of 4 and cols >= nref are refused with a message; the largest cols below nref is taken"""
    tl = PrefixList(5)
    span, win = sw16._draw(tl.rng, 100, 160, 0)
    r, aq = tl.add_read(span, 0, 4, 4)
    off = tl.add_window(win)
    rd = smr.Reads.from_seqs(tl.reads)
    engine.upload_reads(rd, 1)
    rd.free()
    sc = SCHEMES[0]
    n = 0
    for cols, msg in ((0, "must not be 0"), (6, "multiple of 4"), (160, "less than nref"), (164, "less than nref"), (156, None)):
        try:
            got = engine.sw16_prefix_batch([(r, aq, 100, 0, off, 160, cols)], bytes(tl.ref), 19, **sw16._sc(sc))
            assert msg is None, "not refused: cols %d" % cols
            assert got[0].tolist() == interval(span, win, cols, sc)
        except smr.SmrError as e:
            assert msg is not None and msg in str(e), (msg, str(e))
        n += 1
    return n
