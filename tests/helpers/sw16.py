"""k_sw16<13 | 19 | 26 | 32> (smr_walk.hpp) through smr_sw16_batch and the long-read strips through smr_ssw_batch mode 5, against the answers of
the reference's own ssw.c (tests/golden/sw16_pairs.json, ssw_pairs_long.json.gz; written by tests/golden/make_golden_ssw.py --sw16 / --long)
and against the plain DP of helpers/swdp.py on task lists drawn here.  The same bodies run on the GPU (tests/test_gpu_sw16.py) and on the
wave64 emulator (tests/test_emu_sw16.py).  Every check counts the cases it compared and returns that number.  TEST INFRASTRUCTURE."""
import collections
import gzip
import json
import os

import numpy as np

import sortmerna_amd as smr
from . import paths, sswgold, swdp

ROWS = (13, 19, 26, 32)
SCHEMES = [dict(match=2, mismatch=-3, score_N=-3, gap_open=5, gap_ext=2, filters=30), dict(match=5, mismatch=-4, score_N=-4, gap_open=5, gap_ext=2, filters=60)]
_ASCII = "ACGTN"
_TR = bytes.maketrans(b"ACGTN", bytes(range(5)))


def load():
    return sswgold.load("sw16_pairs.json")


def load_long():
    g = json.loads(gzip.open(os.path.join(paths.REPO, "tests", "golden", "ssw_pairs_long.json.gz")).read())
    for c in g["cases"]:
        c["reads_b"] = [s.encode().translate(_TR) for s in c["reads"]]
        c["refs_b"] = [s.encode().translate(_TR) for s in c["refs"]]
        c["expected_a"] = np.array(c["expected"], dtype=np.int32)
    return g["cases"]


def _sc(sc):
    return dict(match=sc["match"], mismatch=sc["mismatch"], score_N=sc["score_N"], gap_open=sc["gap_open"], gap_ext=sc["gap_ext"], filters=sc["filters"])


class TaskList:
    """reads of a batch (as the letters a FASTA file would hold), the letters that stand in for an index part's references, and tasks over them"""

    def __init__(self, seed):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.reads, self.ref, self.tasks, self.expected, self.what = [], bytearray(), [], [], []

    def add_read(self, span, reversed_, pre=0, post=0):
        """a read that holds `span` (0..4 codes) as rows [pre, pre + len) of its forward (reversed_ = 0) or reverse-complement strand; -> (read index, aq)"""
        strand = bytes(self.rng.integers(0, 4, size=pre).astype(np.uint8)) + bytes(span) + bytes(self.rng.integers(0, 4, size=post).astype(np.uint8))
        phys = strand if not reversed_ else bytes(x if x == 4 else 3 - x for x in reversed(strand))
        self.reads.append("".join(_ASCII[x] for x in phys))
        return len(self.reads) - 1, pre

    def add_window(self, window, gap=0):
        self.ref += bytes(self.rng.integers(0, 4, size=gap).astype(np.uint8))      # (letters between windows are never N: a window's N is its own)
        off = len(self.ref)
        self.ref += bytes(window)
        return off

    def add_task(self, read, aq, m, reversed_, win_off, nref, list_b, expected, what):
        self.tasks.append((read, aq, m, reversed_, win_off, nref, list_b))
        self.expected.append(list(expected) if not list_b else [expected[0], -1, -1, -1, -1])
        self.what.append(what)

    def add_problem(self, span, window, expected, reversed_, lists=(0, 1), pre=0, post=0, what=""):
        r, aq = self.add_read(span, reversed_, pre, post)
        off = self.add_window(window, int(self.rng.integers(0, 5)))
        for lb in lists:
            self.add_task(r, aq, len(span), reversed_, off, len(window), lb, expected, what)

    def shuffle(self):
        o = self.rng.permutation(len(self.tasks))
        self.tasks = [self.tasks[i] for i in o]; self.expected = [self.expected[i] for i in o]; self.what = [self.what[i] for i in o]

    def run(self, engine, rows, sc, blocks=0, force_any_n=False):
        rd = smr.Reads.from_seqs(self.reads)
        try:
            engine.upload_reads(rd, 1)
            return engine.sw16_batch(self.tasks, bytes(self.ref), rows, blocks=blocks, force_any_n=force_any_n, **_sc(sc))
        finally:
            rd.free()

    def check(self, engine, rows, sc, blocks=0, force_any_n=False, label=""):
        """-> the number of tasks compared (all of them, or an assertion fails)"""
        got = self.run(engine, rows, sc, blocks, force_any_n)
        assert got.shape == (len(self.tasks), 5)
        n = 0
        for i, t in enumerate(self.tasks):
            assert got[i].tolist() == self.expected[i], "k_sw16<%d> %s scoring %s blocks %d: task %d of %d (%s; read %d of %d letters, aq %d, m %d, reversed %d, window %d letters, list %s): got %s, expected %s" % (
                rows, label, sc, blocks, i, len(self.tasks), self.what[i], t[0], len(self.reads[t[0]]), t[1], t[2], t[3], t[5], "AB"[t[6]], got[i].tolist(), self.expected[i])
            n += 1
        return n


def fixture_size(rows, every=1):
    """tasks check_fixture(rows, every) compares: both strands x both lists of every `every`-th pair whose span the instantiation takes"""
    return sum(4 * len([1 for r in c["reads_b"] if len(r) <= 8 * rows][::every]) for c in load())


def check_fixture(engine, rows, every=1, blocks=0):
    """every pair of sw16_pairs.json with a span of at most 8 x rows letters as four tasks (forward / reverse-complement strand, list A with the begin
    cell / list B score only), inside reads that are longer than the span for two pairs out of three; all tasks of a scheme in one shuffled list"""
    n = 0
    for ci, c in enumerate(load()):
        tl = TaskList(1000 * rows + ci)
        idx = [i for i in range(len(c["reads_b"])) if len(c["reads_b"][i]) <= 8 * rows][::every]
        for k, i in enumerate(idx):
            for rev in (0, 1):
                pre, post = (0, 0) if k % 3 == 0 else (int(tl.rng.integers(0, 70)), int(tl.rng.integers(0, 70))) if k % 3 == 1 else (int(tl.rng.integers(200, 400)), int(tl.rng.integers(0, 40)))
                tl.add_problem(c["reads_b"][i], c["refs_b"][i], c["expected"][i], rev, pre=pre, post=post, what="pair %d of scheme %d" % (i, ci))
        tl.shuffle()
        n += tl.check(engine, rows, c["scoring"], blocks=blocks, label="fixture")
    return n


def check_fixture_through_ssw_batch(engine, modes=(0, 1, 2, 3, 4)):
    """the same stored pairs through the one-pair-per-wave kernels, the four-pair kernel and the striped path (smr_ssw_batch modes 0 - 4): among them the
    pairs without any positive cell (a window of one letter that the read does not hold), for which ssw.c reports read_end1 = 0"""
    n = 0
    for c in load():
        sc = c["scoring"]
        assert any(e[0] == 0 for e in c["expected"]) or sc["mismatch"] == 0
        for mode in modes:
            got = engine.ssw_batch(c["reads_b"], c["refs_b"], mode=mode, **_sc(sc))
            for i, e in enumerate(c["expected"]):
                assert got[i].tolist() == e, "smr_ssw_batch mode %d scoring %s pair %d (m=%d, n=%d): got %s, ssw.c %s" % (mode, sc, i, len(c["reads_b"][i]), len(c["refs_b"][i]), got[i].tolist(), e)
                n += 1
    return n


def check_long(engine, pick=None):
    """smr_ssw_batch mode 5 on the pairs of ssw_pairs_long.json.gz (pick(case index, pair index, m, n, height) -> bool selects; None = all);
    -> (pairs compared, {strip height: different lengths that selected it})"""
    n, heights = 0, collections.defaultdict(set)
    for ci, c in enumerate(load_long()):
        sc = c["scoring"]
        idx = [i for i in range(len(c["reads_b"])) if pick is None or pick(ci, i, len(c["reads_b"][i]), len(c["refs_b"][i]), engine.sw_long_rows(len(c["reads_b"][i])))]
        if not idx:
            continue
        got = engine.ssw_batch([c["reads_b"][i] for i in idx], [c["refs_b"][i] for i in idx], mode=5, **_sc(sc))
        for k, i in enumerate(idx):
            m = len(c["reads_b"][i])
            assert m > 512
            assert got[k].tolist() == c["expected"][i], "long strips (height %d), scoring %s, pair %d (m=%d, n=%d): got %s, ssw.c %s" % (
                engine.sw_long_rows(m), sc, i, m, len(c["refs_b"][i]), got[k].tolist(), c["expected"][i])
            heights[engine.sw_long_rows(m)].add(m)
            n += 1
    return n, {h: len(v) for h, v in heights.items()}


def cheapest_long_pair_per_height(engine):
    """the selector of the emulator's default slice: for every strip height the pair with the fewest cells"""
    best = {}
    for ci, c in enumerate(load_long()):
        for i, (r, f) in enumerate(zip(c["reads_b"], c["refs_b"])):
            h = engine.sw_long_rows(len(r))
            if h not in best or len(r) * len(f) < best[h][0]:
                best[h] = (len(r) * len(f), ci, i)
    keep = {(ci, i) for _, ci, i in best.values()}
    return lambda ci, i, m, n, h: (ci, i) in keep


# ---- task lists drawn here, answers from the plain DP ---------------------------------------------------------------------------------
def _draw(rng, m, n, kind, n_read=True, n_win=True):
    span = rng.integers(0, 4, size=m).astype(np.uint8)
    if n_read:
        span[rng.random(m) < 0.03] = 4
    if kind == 0:                                            # the window holds a noisy copy of the span
        core = [int(x) if x < 4 and rng.random() > 0.08 else int(rng.integers(0, 4)) for x in span if rng.random() > 0.02]
        fl = max(0, n - len(core)) // 2
        win = (list(rng.integers(0, 4, size=fl)) + core + list(rng.integers(0, 4, size=max(0, n - len(core) - fl))))[:n]
        win = np.array(win if win else [0], dtype=np.uint8)
    else:
        win = rng.integers(0, 4, size=n).astype(np.uint8)
    if n_win and win.size > 3:
        win[rng.random(win.size) < 0.02] = 4
    return bytes(span), bytes(win)


def _dp(span, win, sc):
    return swdp.align(span, win, sc["match"], sc["mismatch"], sc["score_N"], sc["gap_open"], sc["gap_ext"], sc["filters"])


N_MIXED = 2 * 44


def check_mixed_waves(engine, rows, sc, seed=1):
    """waves whose sixteen tasks mix spans of 1 and 8 x rows letters, windows of 1 and 600, both strands, spans inside longer reads (also reads of more
    than 256 letters), the shortest read last in the batch; every problem in list A and in list B (whose score must be A's)"""
    tl = TaskList(seed * 100 + rows)
    rng = tl.rng
    top = min(8 * rows, 256)
    shapes = [(1, 1), (1, 600), (top, 1), (top, 600), (top, top), (top - 1, 599), (rows, 600), (rows + 1, 2 * rows), (2, 3), (top, 40)]
    shapes += [(int(rng.integers(1, top + 1)), int(rng.integers(1, 601))) for _ in range(33)]
    for k, (m, n) in enumerate(shapes):
        span, win = _draw(rng, m, n, k % 2, n_read=k % 3 != 2, n_win=k % 4 == 1)
        pre, post = [(0, 0), (int(rng.integers(1, 50)), int(rng.integers(0, 50))), (int(rng.integers(257, 500)), 3), (0, int(rng.integers(257, 300)))][k % 4]
        tl.add_problem(span, win, _dp(span, win, sc), k // 2 % 2, pre=pre, post=post, what="shape %d x %d" % (m, n))
    span, win = _draw(rng, 1, 5, 1, n_read=False, n_win=False)                      # the shortest read, last: the loads behind its record end in the upload's slack
    tl.add_problem(span, win, _dp(span, win, sc), 0, what="one-letter read, last of the batch")
    order = list(rng.permutation(len(tl.tasks)))
    tl.tasks = [tl.tasks[i] for i in order]; tl.expected = [tl.expected[i] for i in order]; tl.what = [tl.what[i] for i in order]
    assert len(tl.tasks) == N_MIXED
    n = tl.check(engine, rows, sc, label="mixed waves")
    by = collections.defaultdict(dict)
    for t, e in zip(tl.tasks, tl.expected):
        by[(t[0], t[1], t[2], t[4])]["AB"[t[6]]] = e[0]
    assert all(v["A"] == v["B"] for v in by.values()) and len(by) * 2 == n
    return n


N_POSITIONS = 16 * 16


def check_every_quad_position(engine, rows, sc, seed=2):
    """one problem in each of the sixteen quad positions of a wave, next to neighbours that differ from wave to wave: the same five numbers"""
    tl = TaskList(seed * 100 + rows)
    rng = tl.rng
    top = min(8 * rows, 256)
    span, win = _draw(rng, top - 3, 2 * top, 0)
    exp = _dp(span, win, sc)
    r0, aq0 = tl.add_read(span, 1, 7, 9)
    off0 = tl.add_window(win)
    pool = []
    for k in range(12):
        s, w = _draw(rng, int(rng.integers(1, top + 1)), int(rng.integers(1, 500)), k % 2, n_win=k % 3 == 0)
        r, aq = tl.add_read(s, k % 2, int(rng.integers(0, 30)), int(rng.integers(0, 30)))
        pool.append((r, aq, len(s), k % 2, tl.add_window(w, 2), len(w), _dp(s, w, sc)))
    for wave in range(16):
        for pos in range(16):
            if pos == wave:
                tl.add_task(r0, aq0, len(span), 1, off0, len(win), 0, exp, "the problem under test at quad %d" % pos)
            else:
                r, aq, m, rev, off, nref, e = pool[int(rng.integers(0, len(pool)))]
                tl.add_task(r, aq, m, rev, off, nref, 0, e, "neighbour")
    assert len(tl.tasks) == N_POSITIONS
    return tl.check(engine, rows, sc, label="quad positions")


N_HASN = 3 * 16


def check_hasn_on_windows_without_n(engine, rows, sc, seed=3):
    """a wave without any N, scored (a) with ref_any_n = 0, (b) with ref_any_n forced to 1 (the window scan finds nothing), (c) after ONE window got an N,
    which switches all sixteen quads of the wave to the instantiation that handles N: the fifteen other tasks must give the same numbers in all three"""
    top = min(8 * rows, 256)
    n = 0
    runs = []
    for variant in range(3):
        tl = TaskList(seed * 100 + rows)                     # (the same seed: the same sixteen problems)
        for k in range(16):
            span, win = _draw(tl.rng, int(tl.rng.integers(1, top + 1)), int(tl.rng.integers(8, 400)), k % 2, n_read=False, n_win=False)
            if variant == 2 and k == 5:
                win = win[:4] + b"\x04" + win[5:]
            tl.add_problem(span, win, _dp(span, win, sc), k % 2, lists=(0,), pre=k, post=16 - k, what="task %d" % k)
        assert (4 in tl.ref) == (variant == 2)
        n += tl.check(engine, rows, sc, force_any_n=variant == 1, label="HASN variant %d" % variant)
        runs.append(tl.expected)
    assert all(runs[0][k] == runs[1][k] == runs[2][k] for k in range(16) if k != 5)
    return n


LIST_SIZES = [(0, 0), (1, 0), (0, 1), (15, 17), (16, 16), (17, 15), (16, 0), (0, 16), (150, 77), (33, 130)]
N_LISTS = sum(a + b for a, b in LIST_SIZES) + 2 * (150 + 77)          # (the 150 + 77 lists run under three grids)


def check_list_sizes_and_grids(engine, rows, sc, seed=4):
    """lists of 0, 1, 15, 16 and 17 tasks (an empty list A or B, a partial last pass) with the product's grid, and lists long enough for several passes per
    block under grids of 3, 2 and 1 blocks (the grid-stride loop with its slot prefetch one pass ahead)"""
    base = TaskList(seed * 100 + rows)
    rng = base.rng
    top = min(8 * rows, 256)
    pool = []
    for k in range(24):
        s, w = _draw(rng, int(rng.integers(1, top + 1)), int(rng.integers(1, 300)), k % 2, n_win=k % 5 == 0)
        r, aq = base.add_read(s, k % 2, int(rng.integers(0, 20)), int(rng.integers(0, 20)))
        pool.append((r, aq, len(s), k % 2, base.add_window(w, 1), len(w), _dp(s, w, sc)))
    n = 0
    for na, nb in LIST_SIZES:
        for blocks in ((3, 2, 1) if (na, nb) == (150, 77) else (3,) if (na, nb) == (33, 130) else (0,)):
            tl = TaskList(0)
            tl.reads, tl.ref = base.reads, base.ref
            for q in range(na + nb):
                r, aq, m, rev, off, nref, e = pool[int(rng.integers(0, len(pool)))]
                tl.add_task(r, aq, m, rev, off, nref, 1 if q >= na else 0, e, "list sizes %d + %d" % (na, nb))
            tl.shuffle()
            n += tl.check(engine, rows, sc, blocks=blocks, label="lists %d + %d" % (na, nb))
    return n


def check_refusals(engine):
    """tasks outside the kernel's stated range are refused, with a message"""
    tl = TaskList(5)
    span, win = _draw(tl.rng, 120, 200, 0)
    r, aq = tl.add_read(span, 0, 4, 4)
    off = tl.add_window(win)
    rd = smr.Reads.from_seqs(tl.reads)
    engine.upload_reads(rd, 1)
    rd.free()
    ok = dict(SCHEMES[0])
    bad = [((r, aq, 120, 0, off, 200, 0), 13, ok, "8 x rows"), ((r, 10, 120, 0, off, 200, 0), 19, ok, "outside the read"), ((r, aq, 120, 0, off + 1, 200, 0), 19, ok, "outside the reference"),
           ((r + 1, aq, 120, 0, off, 200, 0), 19, ok, "outside the batch"), ((r, aq, 0, 0, off, 200, 0), 19, ok, "empty"), ((r, aq, 120, 0, off, 200, 0), 20, ok, "rows must be"),
           ((r, aq, 120, 0, off, 200, 0), 19, dict(ok, gap_open=2, gap_ext=2), "supported range"), ((r, aq, 120, 0, off, 200, 0), 19, dict(ok, match=120, gap_open=200, gap_ext=100), "sw_pk_fits"),
           ((r, aq, 120, 0, off, 200, 0), 19, dict(ok, match=127, mismatch=-127, score_N=-127, gap_open=128, gap_ext=64), None)]
    n = 0
    for task, rows, sc, msg in bad:
        try:
            got = engine.sw16_batch([task], bytes(tl.ref), rows, **_sc(sc))
            assert msg is None, "not refused: %s" % (task,)
            assert got[0].tolist() == _dp(span, win, sc)
        except smr.SmrError as e:
            assert msg is not None and msg in str(e), (msg, str(e))
        n += 1
    return n
