"""k_sw16h<R>, the packed-f16 flavour of k_sw16<R> (smr_walk.hpp, Sw16Ops<true>), through smr_sw16_batch and smr_sw16_prefix_batch: the bodies of
helpers/sw16.py and helpers/sw16_prefix.py with the switch smr_sw16_f16 on and off, the launch counter of k_sw16h as the proof of which kernel
ran, and the shapes those helpers lack (the top of the f16 range, one row, windows shorter than the four-column period, begin-cell tasks),
against the plain DP of helpers/swdp.py.  The same bodies run on the GPU (tests/test_gpu_sw16_f16.py) and on the wave64 emulator
(tests/test_emu_sw16_f16.py).  TEST INFRASTRUCTURE."""
import contextlib

import numpy as np

from . import sw16, sw16_prefix as pfx

SCHEMES = sw16.SCHEMES
# outside sw_h16_fits, inside what k_sw16 takes: the corner scheme of tests/golden/sw16_pairs.json (T = 255, 1, 1), and two whose match + gap_open = 9
# needs four significant bits.  (4/-5/-5/5/2 itself is refused for every Smith-Waterman kernel -- 2 x gap_ext < |mismatch|, scheme_unsupported --
# so the 9 comes with gap_ext = 3 and with mismatch = -4.)
OUTSIDE = [dict(match=127, mismatch=-127, score_N=-127, gap_open=128, gap_ext=64, filters=1000), dict(match=4, mismatch=-5, score_N=-5, gap_open=5, gap_ext=3, filters=30),
           dict(match=4, mismatch=-4, score_N=-4, gap_open=5, gap_ext=2, filters=30)]
REFUSED = dict(match=4, mismatch=-5, score_N=-5, gap_open=5, gap_ext=2, filters=30)


def encodable(v):
    """sw_h16_encodable: the f16 encoding of the integer has a zero low byte (numpy's float16 is the IEEE format)"""
    return 0 <= v <= 2048 and int(np.array([v], dtype=np.float16).view(np.uint16)[0]) & 0xFF == 0


def fits(m, sc):
    """sw_h16_fits as include/smr_hip.h states it"""
    t = [sc[k] + sc["gap_open"] for k in ("match", "mismatch", "score_N")]
    return all(encodable(v) for v in t) and m * sc["match"] + sc["gap_open"] + sc["gap_ext"] + max(t) <= 2048


@contextlib.contextmanager
def flavour(engine, on):
    """inside: the switch as asked; yields a function that tells how many k_sw16h launches happened since"""
    before, _ = engine.sw16_f16()
    mode, n0 = engine.sw16_f16(1 if on else 0)
    assert mode == (1 if on else 0)
    try:
        yield lambda: engine.sw16_f16()[1] - n0
    finally:
        engine.sw16_f16(before)


def expect_launches(count, on, what):
    if on:
        assert count() > 0, "%s: the switch is on and k_sw16h was never launched" % what
    else:
        assert count() == 0, "%s: the switch is off and k_sw16h was launched %d times" % (what, count())


def check_fixture(engine, rows, on):
    """sw16.check_fixture under the switch; the stored corner scheme lies outside sw_h16_fits and takes k_sw16 either way"""
    assert [fits(8 * rows, c["scoring"]) for c in sw16.load()] == [True, True, False, True, True, True]
    with flavour(engine, on) as count:
        n = sw16.check_fixture(engine, rows)
        expect_launches(count, on, "fixture rows %d" % rows)
    return n


def check_drawn(engine, rows, sc, on):
    with flavour(engine, on) as count:
        n = [sw16.check_mixed_waves(engine, rows, sc), sw16.check_every_quad_position(engine, rows, sc), sw16.check_hasn_on_windows_without_n(engine, rows, sc),
             sw16.check_list_sizes_and_grids(engine, rows, sc)]
        expect_launches(count, on, "drawn lists rows %d" % rows)
    assert n == [sw16.N_MIXED, sw16.N_POSITIONS, sw16.N_HASN, sw16.N_LISTS]
    return sum(n)


def check_prefix(engine, rows, sc, on):
    with flavour(engine, on) as count:
        n = [pfx.check_shapes(engine, rows, sc), pfx.check_quads_and_cols(engine, rows, sc)]
        expect_launches(count, on, "prefix rows %d" % rows)
    assert n == [pfx.n_shapes(rows), pfx.N_QUADS]
    return sum(n)


N_EDGES = 2 * 12


def check_edges(engine, sc, on):
    """what the drawn lists lack, every problem with its end and begin cells (list A: the begin cell is a task with rows and columns backwards, dir = -1,
    asked for because the score passes `filters`) and score only (list B), rows 32 for the spans of 256 and rows 19 for the others:
    a perfect match of 256 letters (score 256 x match, the top of the range: 512 under the default scheme); the same with one N in the read and one in
    the window; one row against 1, 3 and 40 columns; windows of one and of three columns (below the four-column period) against 1, 19 and 152 rows"""
    rng = np.random.Generator(np.random.PCG64(77))
    low = dict(sc, filters=1)                               # every positive score gets its begin cell
    n = 0
    for rows, shapes in ((32, ("perfect", "perfect_n")), (19, ((1, 1), (1, 3), (1, 40), (19, 1), (152, 1), (1, 3), (19, 3), (152, 3), (20, 2), (152, 5)))):
        tl = sw16.TaskList(770 + rows)
        for k, shape in enumerate(shapes):
            if shape == "perfect":
                span = bytes(rng.integers(0, 4, size=256).astype(np.uint8)); win = span
            elif shape == "perfect_n":
                span = bytearray(rng.integers(0, 4, size=256).astype(np.uint8)); win = bytearray(span)
                span[100] = 4; win[200] = 4
                span, win = bytes(span), bytes(win)
            else:
                m, nref = shape
                span = bytes(rng.integers(0, 4, size=m).astype(np.uint8))
                win = (span[-nref:] if k % 2 == 0 else span[:nref]).ljust(nref, b"\x01") if nref <= m else bytes(rng.integers(0, 4, size=nref - m).astype(np.uint8)) + span
            exp = sw16._dp(span, win, low)
            if shape == "perfect":
                assert exp == [256 * sc["match"], 0, 255, 0, 255]
            tl.add_problem(span, win, exp, k % 2, pre=3 * k, post=k, what="edge %s" % (shape,))
        assert any(e[0] > 0 and e[1] >= 0 for e in tl.expected)      # (begin cells were asked for)
        with flavour(engine, on) as count:
            n += tl.check(engine, rows, low, label="edges")
            expect_launches(count, on, "edges rows %d" % rows)
    assert n == N_EDGES
    return n


def check_outside(engine):
    """schemes outside sw_h16_fits with the switch ON: no launch of k_sw16h, the answers are the plain DP's (k_sw16 did the work)"""
    n = 0
    for si, sc in enumerate(OUTSIDE):
        assert not fits(152, sc)
        tl = sw16.TaskList(900 + si)
        for k, (m, nref) in enumerate(((152, 200), (60, 90), (1, 7), (100, 3))):
            span, win = sw16._draw(tl.rng, m, nref, k % 2)
            tl.add_problem(span, win, sw16._dp(span, win, sc), k % 2, pre=k, post=2 * k, what="outside scheme %d" % si)
        with flavour(engine, True) as count:
            n += tl.check(engine, 19, sc, label="outside the f16 range")
            assert count() == 0, "scheme %s lies outside sw_h16_fits and k_sw16h was launched" % (sc,)
    return n
