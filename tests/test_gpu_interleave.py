"""smr_interleave_batch: k_mates_zip (csrc/smr_mates.hpp) at its seam.  Piece i of stream A and piece i of stream B, given by the host with
their offsets, come back as a[0] + b[0] + a[1] + b[1] + ...  The yardstick is Python's b"".join, never the code under test.

The kernel's constants that the cases are built around (named here, asserted against nothing but the join): a wave takes GROUP = 64
consecutive pairs, a team of 16 lanes TEAM = 16 of them, and a piece longer than TEAM_BYTES = 1024 makes the whole wave stream its group; the
offsets are looked up per block of ROWS_BLOCK = 256 pairs.

test_emu_interleave.py runs the same bodies on the kernel emulator, where device memory lies between guard pages: a store behind the last
byte of the output (allocated at exactly `need` bytes by the seam) faults at once."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_state_import import engine

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY = -1, -4
COUNTS = [1, 63, 64, 65, 255, 256, 257, 1025]
GROUP, TEAM, TEAM_BYTES, ROWS_BLOCK = 64, 16, 1024, 256


def fill(rng, n):
    return rng.integers(1, 255, n, dtype=np.uint8).tobytes()


def draw_lengths(rng, n, long_at=None, huge_at=None):
    """per piece: 0 with probability 0.8, else 1..9 or 60..400; one piece above 8192 and one above 70 000 where asked for"""
    kind = rng.random(n)
    small = rng.integers(1, 10, n)
    mid = rng.integers(60, 401, n)
    lens = np.where(kind < 0.8, 0, np.where(kind < 0.9, small, mid)).astype(np.int64)
    if long_at is not None:
        lens[long_at] = 8192 + int(rng.integers(1, 700))
    if huge_at is not None:
        lens[huge_at] = 70000 + int(rng.integers(1, 700))
    return [int(x) for x in lens]


def draw(n, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    la = draw_lengths(rng, n, long_at=n // 3 if n >= 63 else None, huge_at=(2 * n) // 3 if n >= 255 else None)
    lb = draw_lengths(rng, n, long_at=n // 2 if n >= 63 else None, huge_at=n // 5 if n >= 255 else None)
    return [fill(rng, k) for k in la], [fill(rng, k) for k in lb]


def join(a, b):
    return b"".join(x + y for x, y in zip(a, b))


def phases(a, b):
    """(source start mod 4, destination start mod 4) of every piece that is not empty, per source"""
    seen = {0: set(), 1: set()}
    sa = sb = d = 0
    for x, y in zip(a, b):
        if x:
            seen[0].add((sa % 4, d % 4))
        sa += len(x); d += len(x)
        if y:
            seen[1].add((sb % 4, d % 4))
        sb += len(y); d += len(y)
    return seen


def random_body(n):
    e = engine()
    try:
        a, b = draw(n, seed=1000 + n)
        assert e.interleave_batch(a, b) == join(a, b)
        if n >= 255:
            assert max(map(len, a)) > 70000 and max(map(len, b)) > 70000 and sum(1 for x in a + b if 8192 < len(x) < 70000) >= 2
            assert sum(1 for x in a + b if not x) > 1.4 * n
    finally:
        e.close()


@pytest.mark.parametrize("n", COUNTS)
def test_random_pieces_equal_the_join(n):
    random_body(n)


def empties_body():
    e = engine()
    try:
        rng = np.random.Generator(np.random.PCG64(7))
        for n in (1, 65, 257):
            none = [b""] * n
            some = [fill(rng, int(k)) for k in rng.integers(0, 300, n)]
            some[0] = some[0] or b"x"
            assert e.interleave_batch(none, none) == b""
            assert e.interleave_batch(none, some) == b"".join(some)
            assert e.interleave_batch(some, none) == b"".join(some)
    finally:
        e.close()


def test_all_pieces_empty_and_one_stream_empty():
    empties_body()


def phases_body():
    """every (source start mod 4, destination start mod 4) for both sources, in the team path (short pieces) and in the wide path"""
    e = engine()
    try:
        rng = np.random.Generator(np.random.PCG64(11))
        for long_piece in (0, 3000):
            la = [int(x) for x in rng.integers(0, 40, 520)]
            lb = [int(x) for x in rng.integers(0, 40, 520)]
            if long_piece:
                for k in range(0, 520, 7):          # a long piece in every group: the whole wave takes it
                    la[k] = long_piece + k
                    lb[(k + 3) % 520] = long_piece + 2 * k + 1
            a, b = [fill(rng, k) for k in la], [fill(rng, k) for k in lb]
            seen = phases(a, b)
            assert len(seen[0]) == 16 and len(seen[1]) == 16, (long_piece, seen)
            assert e.interleave_batch(a, b) == join(a, b)
    finally:
        e.close()


def test_every_source_and_destination_phase():
    phases_body()


def boundaries_body():
    """pieces of TEAM_BYTES - 1, TEAM_BYTES, TEAM_BYTES + 1 bytes (the last one makes its group wide) in either stream, at the first and last
    pair of a team, of a group and of an offset block; and teams / groups whose output ends exactly on, one byte before and one byte behind a
    dword that the next team begins in"""
    e = engine()
    try:
        rng = np.random.Generator(np.random.PCG64(13))
        n = 2 * ROWS_BLOCK + GROUP + 3
        spots = [0, TEAM - 1, TEAM, GROUP - 1, GROUP, GROUP + TEAM - 1, ROWS_BLOCK - 1, ROWS_BLOCK, 2 * ROWS_BLOCK - 1, 2 * ROWS_BLOCK, n - 1]
        for size in (TEAM_BYTES - 1, TEAM_BYTES, TEAM_BYTES + 1, 4 * TEAM_BYTES, 4 * TEAM_BYTES + 1):
            for stream in (0, 1):
                for pad in (0, 1, 2, 3):
                    lens = [[0] * n, [0] * n]
                    for k, s in enumerate(spots):
                        lens[(stream + k) % 2][s] = size
                        if s + 1 < n:
                            lens[(stream + k + 1) % 2][s + 1] = 5 + (k % 4)       # a short neighbour in the next pair
                    lens[1 - stream][0] = pad                                          # shifts every later boundary by one byte
                    a, b = [fill(rng, k) for k in lens[0]], [fill(rng, k) for k in lens[1]]
                    assert e.interleave_batch(a, b) == join(a, b), (size, stream, pad)
    finally:
        e.close()


def test_pieces_at_the_team_and_group_boundaries():
    boundaries_body()


def raw_call(e, a, b, buf, cap, a_off=None, b_off=None):
    n = len(a)
    a_off = np.array(a_off if a_off is not None else np.concatenate([[0], np.cumsum([len(x) for x in a])]), dtype=np.uint64)
    b_off = np.array(b_off if b_off is not None else np.concatenate([[0], np.cumsum([len(x) for x in b])]), dtype=np.uint64)
    ab = np.frombuffer(b"".join(a) or b"\0", dtype=np.uint8)
    bb = np.frombuffer(b"".join(b) or b"\0", dtype=np.uint8)
    u64p = C.POINTER(C.c_uint64)
    need = C.c_uint64(9)
    rc = e.L.smr_interleave_batch(e.h, n, ab.ctypes.data, a_off.ctypes.data_as(u64p), bb.ctypes.data, b_off.ctypes.data_as(u64p),
                                  buf.ctypes.data if buf is not None else None, cap, C.byref(need))
    return rc, need.value


def contract_body():
    e = engine()
    try:
        for seed, n in ((21, 65), (22, 257), (23, 300)):
            a, b = draw(n, seed)
            if seed == 23:                       # the output ends one, two, three bytes into its last dword
                a[-1], b[-1] = b"abc", b"de"
            want = join(a, b)
            rc, need = raw_call(e, a, b, None, 0)
            assert rc == 0 and need == len(want)
            buf = np.full(need + 64, 0x5A, dtype=np.uint8)
            rc, need2 = raw_call(e, a, b, buf, need - 1)
            assert rc == ERR_CAPACITY and need2 == need and (buf == 0x5A).all()
            assert "smr_interleave_batch" in e.L.smr_last_error(e.h).decode()
            rc, need2 = raw_call(e, a, b, buf, need)
            assert rc == 0 and need2 == need and buf[:need].tobytes() == want and (buf[need:] == 0x5A).all()
        for tail in (1, 2, 3, 4, 5):             # the last dword of the output: nothing behind `need`
            a, b = [b"x" * 40, b""], [b"", b"y" * tail]
            buf = np.full(40 + tail + 16, 0x5A, dtype=np.uint8)
            rc, need = raw_call(e, a, b, buf, 40 + tail)
            assert rc == 0 and buf[:need].tobytes() == join(a, b) and (buf[need:] == 0x5A).all()
        # n = 0, and offsets that decrease
        need = C.c_uint64(9)
        assert e.L.smr_interleave_batch(e.h, 0, None, None, None, None, None, 0, C.byref(need)) == 0 and need.value == 0
        a, b = [b"abcd", b"ef"], [b"g", b"hij"]
        buf = np.full(64, 0x5A, dtype=np.uint8)
        assert raw_call(e, a, b, buf, 64, a_off=[0, 4, 3])[0] == ERR_ARG and (buf == 0x5A).all()
        assert raw_call(e, a, b, buf, 64, b_off=[2, 1, 4])[0] == ERR_ARG and (buf == 0x5A).all()
        # offsets that do not start at 0
        rc, need = raw_call(e, [b"abcd", b"ef"], b, buf, 64, a_off=[1, 4, 6])
        assert rc == 0 and buf[:need].tobytes() == b"bcd" + b"g" + b"ef" + b"hij"
        assert e.interleave_batch(a, b) == join(a, b)          # the context goes on working
    finally:
        e.close()


def test_sizes_capacity_guard_bytes_and_refusals():
    contract_body()
