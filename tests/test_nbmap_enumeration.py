"""CPU: the candidate list of the search bitmap's builder (csrc/smr_nbmap.hpp::nb_candidate, mirrored by helpers/nbmap.py) is COMPLETE.

The builder sets bit proj(P) of a mini-trie's slab for every candidate P of every string T that lev1_entry accepts; k_seed_pg then skips a
search whose bit is clear.  A pattern that accepts T but is missing from T's list would lose hits, so: for pw = 4 and 5 every pair (P, T) is
checked, for pw = 9 and 10 a million near-matches (0, 1 or 2 edits apart) and a million random pairs, against the closed form of the
automaton restated from tests/test_lev_closed_form.py (which proves it equal to the reference's tables)."""
import numpy as np
import pytest

from helpers import nbmap


@pytest.mark.parametrize("pw", [4, 5])
def test_enumerate_then_verify_gives_exactly_the_accepted_pairs(pw):
    nT, nP = 1 << (2 * (pw + 1)), 1 << (2 * pw)
    T = np.arange(nT, dtype=np.uint64)
    want = nbmap.accepts(np.arange(nP, dtype=np.uint64)[None, :], T[:, None], pw)        # [T, P]
    C = nbmap.candidates(T, pw)
    ok = nbmap.accepts(C, T[:, None], pw)
    got = np.zeros((nT, nP), dtype=bool)
    rows = np.broadcast_to(np.arange(nT)[:, None], C.shape)
    got[rows[ok], C[ok]] = True
    assert want.sum() > nT                                   # (every string accepts its own prefix and more)
    assert np.array_equal(got, want)
    # a projected bitmap covers every accepted pair: bit proj(P) of a "mini-trie" {T} is set for every P that accepts T
    tt, pp = np.nonzero(want)
    for drop in (1, 2):
        keep = (1 << (2 * (pw - drop))) - 1
        bits = np.zeros((nT, keep + 1), dtype=bool)
        bits[rows[ok], C[ok] & keep] = True
        assert bits[tt, pp & keep].all()
        # ... and is exactly the projection: no bit without an accepted pattern under it
        proj = np.zeros_like(bits)
        proj[tt, pp & keep] = True
        assert np.array_equal(bits, proj)


def _edited(rng, T, pw, n):
    """patterns 0, 1 or 2 edits away from their strings: the first pw chars of T after a substitution, a deletion or an insertion, and for half of
    them a second substitution"""
    t = ((T[:, None] >> (2 * np.arange(pw + 1, dtype=np.uint64))) & np.uint64(3)).astype(np.int64)      # [n, pw + 1] chars
    op = rng.integers(0, 4, n)
    j = rng.integers(0, pw, n)
    x = rng.integers(0, 4, n)
    col = np.arange(pw)[None, :]
    p = t[:, :pw].copy()
    sub = op == 1
    p[sub, j[sub]] = x[sub]
    dele = np.take_along_axis(t, col + (col >= j[:, None]), axis=1)                                  # char j of T removed
    p[op == 2] = dele[op == 2]
    ins = np.take_along_axis(t, col - (col > j[:, None]), axis=1)                                    # x put in at position j
    ins[np.arange(n), j] = x
    p[op == 3] = ins[op == 3]
    second = rng.random(n) < 0.5
    j2, x2 = rng.integers(0, pw, n), rng.integers(0, 4, n)
    p[second, j2[second]] = x2[second]
    return (p.astype(np.uint64) << (2 * np.arange(pw, dtype=np.uint64))[None, :]).sum(axis=1).astype(np.uint64)


@pytest.mark.parametrize("pw", [9, 10])
def test_no_accepted_pattern_is_missing_from_the_list(pw):
    rng = np.random.Generator(np.random.PCG64(1000 + pw))
    n = 1_000_000
    seen = 0
    for kind in ("near", "random"):
        T = rng.integers(0, 1 << (2 * (pw + 1)), n, dtype=np.uint64)
        P = _edited(rng, T, pw, n) if kind == "near" else rng.integers(0, 1 << (2 * pw), n, dtype=np.uint64)
        want = nbmap.accepts(P, T, pw)
        got = np.zeros(n, dtype=bool)
        for lo in range(0, n, 100_000):
            C = nbmap.candidates(T[lo:lo + 100_000], pw)
            ok = nbmap.accepts(C, T[lo:lo + 100_000, None], pw)
            got[lo:lo + 100_000] = (ok & (C == P[lo:lo + 100_000, None].astype(np.uint32))).any(axis=1)
        assert np.array_equal(got, want), "%s pairs, pw %d: %d differ" % (kind, pw, int((got != want).sum()))
        if kind == "near":
            assert 0.4 * n < want.sum() < 0.9 * n            # the sample has both kinds
        seen += int(want.sum())
    assert seen > 0
