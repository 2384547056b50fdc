"""A plain affine-gap Smith-Waterman in numpy with 64-bit integers: the textbook recurrence

    E[i][j] = max(E[i][j-1] - gap_ext, H[i][j-1] - gap_open)        (a gap that runs along the reference)
    F[i][j] = max(F[i-1][j] - gap_ext, H[i-1][j] - gap_open)        (a gap that runs along the read)
    H[i][j] = max(0, H[i-1][j-1] + s(read[i], ref[j]), E[i][j], F[i][j])

filled one anti-diagonal at a time (a cell needs only the two diagonals before its own, so nothing about the order is assumed of the
scheme).  Sequences are in the 0..4 alphabet; s = score_N when either letter is 4, else match / mismatch.  The end cell is the one ssw_align
reports: the EARLIEST reference column that reaches the maximum and the smallest read row in it; the begin cell is the end cell of the same
recurrence over the reversed prefixes that end in the end cell.  TEST INFRASTRUCTURE: the reference the kernels' answers are compared with
where no stored answer of ssw.c exists (tests/test_host_cpu.py asserts that it returns ssw.c's five numbers on every stored pair)."""
import numpy as np

NEG = -(1 << 40)


def fill(read, ref, match, mismatch, score_N, gap_open, gap_ext):
    """-> H as an (m, n) int64 array"""
    a = np.frombuffer(bytes(read), dtype=np.uint8).astype(np.int64)
    b = np.frombuffer(bytes(ref), dtype=np.uint8).astype(np.int64)
    m, n = a.size, b.size
    S = np.where(a[:, None] == b[None, :], match, mismatch).astype(np.int64)
    S[a == 4, :] = score_N
    S[:, b == 4] = score_N
    H = np.zeros((m + 1, n + 1), dtype=np.int64)
    E = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    F = np.full((m + 1, n + 1), NEG, dtype=np.int64)
    for d in range(2, m + n + 1):
        i = np.arange(max(1, d - n), min(m, d - 1) + 1)
        j = d - i
        e = np.maximum(E[i, j - 1] - gap_ext, H[i, j - 1] - gap_open)
        f = np.maximum(F[i - 1, j] - gap_ext, H[i - 1, j] - gap_open)
        h = np.maximum(np.maximum(H[i - 1, j - 1] + S[i - 1, j - 1], 0), np.maximum(e, f))
        E[i, j] = e
        F[i, j] = f
        H[i, j] = h
    return H[1:, 1:]


def end_cell(H):
    """(score, column, row): the earliest column that holds the maximum, the smallest row in it"""
    best = int(H.max()) if H.size else 0
    if best <= 0:
        return 0, -1, 0              # (no column reaches a positive score: ssw_align leaves ref_end1 at -1 and its end-row scan meets a column of zeros, row 0 first)
    col = int(np.argmax(H.max(axis=0) == best))
    row = int(np.argmax(H[:, col] == best))
    return best, col, row


def align(read, ref, match, mismatch, score_N, gap_open, gap_ext, filters=0):
    """-> [score1, ref_begin1, ref_end1, read_begin1, read_end1] as ssw_align(flag 2) returns them (begins -1 below `filters`)"""
    sc = (match, mismatch, score_N, gap_open, gap_ext)
    score, ec, er = end_cell(fill(read, ref, *sc))
    out = [min(score, 65535), -1, ec, -1, er]
    if score > 0 and out[0] >= filters:
        s2, bc, br = end_cell(fill(bytes(read[:er + 1])[::-1], bytes(ref[:ec + 1])[::-1], *sc))
        assert s2 == score, (s2, score)
        out[1], out[3] = ec - bc, er - br
    return out


def score_only(read, ref, match, mismatch, score_N, gap_open, gap_ext):
    return min(int(max(fill(read, ref, match, mismatch, score_N, gap_open, gap_ext).max(), 0)), 65535)
