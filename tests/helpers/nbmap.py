"""The search bitmap of csrc/smr_nbmap.hpp restated with numpy: the patterns a string accepts (nb_candidate), the closed form of the LEV(1)
automaton they are verified with (tests/test_lev_closed_form.py::closed_form, on arrays), and the slabs of a part from its pigeonhole layout.
Strings and patterns are 2 bits per char, char i at bits 2i; a string T has pw + 1 chars, a pattern P has pw."""
import numpy as np

NONE = 0xFFFFFFFF


def accepts(P, T, pw):
    """bool[...]: does pattern P accept string T (a + s2 >= pw-1 or a + s0 >= pw-1 or a + s1 >= pw: the run form of the closed form)"""
    P = np.asarray(P, dtype=np.uint64)
    T = np.asarray(T, dtype=np.uint64)

    def ch(v, i):
        return (v >> np.uint64(2 * i)) & np.uint64(3)

    eq0 = [ch(P, i) == ch(T, i) for i in range(pw)]
    eq1 = [ch(P, i) == ch(T, i + 1) for i in range(pw)]
    eq2 = [ch(P, i + 1) == ch(T, i) for i in range(pw - 1)]

    def lead(v):
        n = np.zeros(np.broadcast(P, T).shape, dtype=np.int64)
        run = np.ones(n.shape, dtype=bool)
        for e in v:
            run = run & e
            n += run
        return n

    a, s0, s1, s2 = lead(eq0), lead(eq0[::-1]), lead(eq1[::-1]), lead(eq2[::-1])
    return (a + s2 >= pw - 1) | (a + s0 >= pw - 1) | (a + s1 >= pw)


def n_candidates(pw):
    return 8 * pw + 2


def candidates(T, pw):
    """uint32[len(T), 8 pw + 2]: nb_candidate(T, pw, c) for every c, in the builder's order"""
    T = np.asarray(T, dtype=np.uint64).reshape(-1)
    m = np.uint64((1 << (2 * pw)) - 1)
    cols = [T & m]
    for pos in range(pw):
        for x in (1, 2, 3):
            cols.append((T & m) ^ np.uint64(x << (2 * pos)))
    for j in range(pw + 1):
        lo = np.uint64((1 << (2 * j)) - 1)
        cols.append(((T & lo) | ((T >> np.uint64(2)) & ~lo)) & m)
    for j in range(pw):
        lo = np.uint64((1 << (2 * j)) - 1)
        for x in range(4):
            cols.append(((T & lo) | np.uint64(x << (2 * j)) | ((T & ~lo) << np.uint64(2))) & m)
    out = np.stack(cols, axis=1).astype(np.uint32)
    assert out.shape[1] == n_candidates(pw)
    return out


def slab_words(pw, drop):
    return (1 << (2 * (pw - drop))) // 32


def strings_of_block(pg, rx, ry):
    """the n strings of a block's TA copy (pg_strings_at): behind the two directories when the block has them"""
    n, cA, cB = ry & 0xFFFFFF, (ry >> 24) & 15, ry >> 28
    at = int(rx) * 4 + ((1 << (2 * cA)) + (1 << (2 * cB)) + 2 if cA else 0)
    return np.asarray(pg[at:at + n], dtype=np.uint32)


def host_slabs(pg, root3, pw, drop, blocks, brute=False):
    """uint32[len(blocks), slab_words]: the slabs of the block table entries `blocks` (2 * key + direction) from the part's host-built layout.
    brute: every pattern against every string of the block (small pw only); otherwise the candidates of every string, verified"""
    bits = 2 * (pw - drop)
    out = np.zeros((len(blocks), 1 << bits), dtype=bool)
    allP = np.arange(1 << (2 * pw), dtype=np.uint64) if brute else None
    for k, i in enumerate(blocks):
        rx, ry = int(root3[2 * i]), int(root3[2 * i + 1])
        if rx == NONE:
            continue
        T = strings_of_block(pg, rx, ry).astype(np.uint64)
        if brute:
            P = allP[accepts(allP[None, :], T[:, None], pw).any(axis=0)]
        else:
            C = candidates(T, pw)
            P = C[accepts(C, T[:, None], pw)].astype(np.uint64)
        out[k, (P & np.uint64((1 << bits) - 1)).astype(np.int64)] = True
    return np.packbits(out.reshape(len(blocks), -1, 32), axis=-1, bitorder="little").view(np.uint32).reshape(len(blocks), -1)
