"""TEST INFRASTRUCTURE: the bodies of the tests of the line-cut gzip path -- smr_gzip_lines_batch (test_gpu_gzip_lines.py / test_emu_gzip_lines.py)
and smr_rows_part_gz / smr_pairwise_part_gz (test_gpu_rows_gz.py / test_emu_rows_gz.py); each body runs on the GPU and on the kernel emulator.

Every yardstick is Python's zlib, which inflates the device's output member by member (that checks the DEFLATE data, each member's CRC-32 and
ISIZE), the plain sibling of a _gz call, and a model of the cut rule written here -- never the code under test."""
import ctypes as C
import random
import zlib

import numpy as np

import sortmerna_amd as smr
from sortmerna_amd import capi

from . import golden, rows

ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -4, -5
PITCH, WIN = 48 * 1024, 16 * 1024


# ------------------------------------------------------------------------------------------------ yardsticks
def members(blob):
    """the gzip members of blob, each inflated by zlib -> [plain bytes]"""
    out = []
    while blob:
        d = zlib.decompressobj(31)
        plain = d.decompress(blob) + d.flush()
        assert d.eof, "a member that does not end"
        out.append(plain)
        blob = d.unused_data
    return out


def model_cuts(data):
    """where the members of `data` end: nominal cut j at b = (j + 1) * PITCH moves to behind the last newline of data[b - WIN:b], and stays at
    b when there is none -> (ends, found): the end of every member, and for every member but the last whether a newline was found"""
    n = len(data)
    ends, found = [], []
    for j in range((n + PITCH - 1) // PITCH - 1):
        b = (j + 1) * PITCH
        p = data.rfind(b"\n", b - WIN, b)
        ends.append(p + 1 if p >= 0 else b)
        found.append(p >= 0)
    return ends + ([n] if n else []), found


def check(data, out, what):
    """`out` is `data` as gzip members that end where the model says"""
    if not data:
        assert out == b"", "%s: an empty stream produces bytes" % what
        return []
    got = members(out)
    assert b"".join(got) == data, "%s: does not inflate to the input" % what
    assert len(got) == (len(data) + PITCH - 1) // PITCH, "%s: %d members for %d bytes" % (what, len(got), len(data))
    assert max(len(m) for m in got) <= 65536, "%s: a member of %d plain bytes" % (what, max(len(m) for m in got))
    ends, found = model_cuts(data)
    at = 0
    for j, m in enumerate(got):
        at += len(m)
        assert at == ends[j], "%s: member %d ends at %d, the rule says %d" % (what, j, at, ends[j])
        if j < len(found):
            assert m.endswith(b"\n") == found[j], "%s: member %d ends in a newline: %s, the rule says %s" % (what, j, m.endswith(b"\n"), found[j])
    assert out[:8] == b"\x1f\x8b\x08\x00\x00\x00\x00\x00", "%s: a header with a name, flags or an mtime" % what
    return got


def filler(n, seed):
    """n bytes of letters without a newline"""
    rng = random.Random(seed)
    words = [bytes(rng.choice(b"ACGTNacgt\t0123456789") for _ in range(3 + rng.randrange(20))) for _ in range(40)]
    out = bytearray()
    while len(out) < n:
        out += words[rng.randrange(40)]
    return bytes(out[:n])


def with_newlines(n, at, seed):
    t = bytearray(filler(n, seed))
    for p in at:
        t[p] = 10
    return bytes(t)


def short_lines(n, seed):
    rng = random.Random(seed)
    out = bytearray()
    while len(out) < n:
        out += filler(1 + rng.randrange(120), rng.randrange(1 << 30)) + b"\n"
    return bytes(out[:n - 1]) + b"\n"


_texts = {}
TEXT_NAMES = ["lines of 100 bytes over 200 KiB", "PITCH bytes that end in a newline", "PITCH bytes and one more", "a newline at b - WIN",
              "a newline at b - WIN - 1", "a newline at b - 1", "no newline over 150 KiB", "a line of 40 KiB among short lines", "empty lines only"]


def texts():
    if _texts:
        return _texts
    t = _texts
    t[TEXT_NAMES[0]] = b"".join(filler(99, k % 50) + b"\n" for k in range(2048))
    t[TEXT_NAMES[1]] = short_lines(PITCH, 2)
    t[TEXT_NAMES[2]] = short_lines(PITCH, 2) + b"x"
    t[TEXT_NAMES[3]] = with_newlines(2 * PITCH + 1000, [PITCH - WIN, 2 * PITCH - WIN], 4)
    t[TEXT_NAMES[4]] = with_newlines(2 * PITCH + 1000, [PITCH - WIN - 1, 2 * PITCH - WIN - 1], 5)
    t[TEXT_NAMES[5]] = with_newlines(2 * PITCH + 1000, [PITCH - 1, 2 * PITCH - 1], 6)
    t[TEXT_NAMES[6]] = filler(150 * 1024, 7)
    t[TEXT_NAMES[7]] = short_lines(30000, 8) + filler(40 * 1024 - 1, 9) + b"\n" + short_lines(150 * 1024 - 30000 - 40 * 1024, 10)
    t[TEXT_NAMES[8]] = b"\n" * (2 * PITCH + 5)
    assert list(t) == TEXT_NAMES
    # what the texts must hold for the tests to show anything
    assert len(t[TEXT_NAMES[0]]) == 204800 and all(len(l) == 99 for l in t[TEXT_NAMES[0]].split(b"\n")[:-1])
    assert len(t[TEXT_NAMES[1]]) == PITCH and t[TEXT_NAMES[1]].endswith(b"\n")
    assert model_cuts(t[TEXT_NAMES[2]])[0] == [PITCH, PITCH + 1]
    assert model_cuts(t[TEXT_NAMES[3]]) == ([PITCH - WIN + 1, 2 * PITCH - WIN + 1, 2 * PITCH + 1000], [True, True])
    assert model_cuts(t[TEXT_NAMES[4]]) == ([PITCH, 2 * PITCH, 2 * PITCH + 1000], [False, False])          # hard cuts
    assert model_cuts(t[TEXT_NAMES[5]]) == ([PITCH, 2 * PITCH, 2 * PITCH + 1000], [True, True])
    assert model_cuts(t[TEXT_NAMES[6]])[1] == [False] * 3
    assert model_cuts(t[TEXT_NAMES[7]])[1] == [False, True, True] and len(t[TEXT_NAMES[7]]) == 150 * 1024  # the window of the first cut lies inside the long line
    return t


def eight_streams():
    """a 1-byte stream and empty streams among streams of one, two and several members"""
    t = texts()
    return [t[TEXT_NAMES[7]], b"", b"x", t[TEXT_NAMES[2]], b"", t[TEXT_NAMES[4]], b"\n", t[TEXT_NAMES[1]]]


# ------------------------------------------------------------------------------------------------ smr_gzip_lines_batch
def _raw_call(e, streams, buf, cap):
    n = len(streams)
    off = (C.c_uint64 * (n + 1))()
    for k in range(n):
        off[k + 1] = off[k] + len(streams[k])
    plain = np.frombuffer(b"".join(streams) or b"\0", dtype=np.uint8)
    gz_off, need = (C.c_uint64 * (n + 1))(*([7] * (n + 1))), C.c_uint64(7)
    rc = e.L.smr_gzip_lines_batch(e.h, plain.ctypes.data, off, n, buf.ctypes.data if buf is not None else None, cap, gz_off, C.byref(need))
    return rc, [int(x) for x in gz_off], need.value


def contract(e, streams, what):
    """sizes only, one byte short, the bound, twice the same bytes -> the members of every stream"""
    total_plain = sum(len(s) for s in streams)
    bound = e.gzip_lines_bound(total_plain, len(streams))
    rc, offs, need = _raw_call(e, streams, None, 0)
    assert rc == 0 and offs[0] == 0 and offs[-1] == need, "%s: sizes only: rc %d, %s, %d" % (what, rc, offs, need)
    print("%s: %d plain bytes -> %d, the bound is %d" % (what, total_plain, need, bound))
    assert need <= bound, "%s: %d bytes, smr_gzip_lines_bound says %d" % (what, need, bound)
    buf = np.full(need + 64, 0xA5, dtype=np.uint8)
    if need:
        rc, offs2, need2 = _raw_call(e, streams, buf, need - 1)
        assert rc == ERR_CAPACITY and offs2 == offs and need2 == need and (buf == 0xA5).all(), "%s: one byte short" % what
        assert b"smr_gzip_lines_batch" in e.L.smr_last_error(e.h)
    rc, offs2, need2 = _raw_call(e, streams, buf, need + 64)
    assert rc == 0 and offs2 == offs and need2 == need and (buf[need:] == 0xA5).all(), "%s: the writing call" % what
    first = buf[:need].tobytes()
    buf[:] = 0xA5
    rc, offs2, need2 = _raw_call(e, streams, buf, need)
    assert rc == 0 and offs2 == offs and buf[:need].tobytes() == first, "%s: two calls, two outputs" % what
    return [first[offs[k]:offs[k + 1]] for k in range(len(streams))]


def text_body(name):
    e = smr.Engine(0)
    try:
        data = texts()[name]
        out = contract(e, [data], name)[0]
        check(data, out, name)
        assert e.gzip_lines_batch([data])[0] == out
    finally:
        e.close()


def eight_streams_body():
    e = smr.Engine(0)
    try:
        s = eight_streams()
        out = contract(e, s, "eight streams")
        for k in range(8):
            check(s[k], out[k], "stream %d of eight" % k)
        assert out[1] == out[4] == b"" and len(members(out[2])) == 1
        assert e.gzip_lines_batch([s[5]])[0] == out[5], "a stream alone differs from the same bytes among eight"
        ms = e.gzip_times()
        assert set(ms) == {"match", "codes", "encode", "compact", "d2h"} and all(v >= 0 for v in ms.values())
    finally:
        e.close()


def arguments_body():
    e = smr.Engine(0)
    L = e.L
    try:
        data = np.frombuffer(texts()[TEXT_NAMES[1]], dtype=np.uint8)
        off = (C.c_uint64 * 2)(0, len(data))
        gz_off, need = (C.c_uint64 * 2)(), C.c_uint64()
        assert L.smr_gzip_lines_batch(e.h, data.ctypes.data, None, 1, None, 0, gz_off, C.byref(need)) == ERR_ARG
        assert L.smr_gzip_lines_batch(e.h, data.ctypes.data, off, 1, None, 0, None, C.byref(need)) == ERR_ARG
        assert L.smr_gzip_lines_batch(e.h, data.ctypes.data, off, 1, None, 0, gz_off, None) == ERR_ARG
        assert L.smr_gzip_lines_batch(e.h, data.ctypes.data, (C.c_uint64 * 2)(5, 4), 1, None, 0, gz_off, C.byref(need)) == ERR_ARG
        assert b"smr_gzip_lines_batch" in L.smr_last_error(e.h)
        for n, k in ((0, 1), (1, 1), (PITCH, 1), (PITCH + 1, 3), (10 * PITCH - 1, 8)):
            assert int(L.smr_gzip_lines_bound(n, k)) == int(L.smr_gzip_bound(n, n // PITCH + k))
        assert e.gzip_lines_batch([]) == [] and e.gzip_lines_batch([b""]) == [b""]
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ smr_rows_part_gz / smr_pairwise_part_gz
def inflate(blob):
    return b"".join(members(blob))


def stream_check(e, plain, gz, what, whole_lines=True):
    """the members of one stream of a _gz call against the sibling's stream"""
    assert bool(gz) == bool(plain), "%s: %d plain bytes, %d compressed" % (what, len(plain), len(gz))
    got = check(plain, gz, what)
    if len(plain) >= 4096:
        assert len(gz) < len(plain), "%s: %d bytes became %d" % (what, len(plain), len(gz))
    if whole_lines:
        assert all(m.endswith(b"\n") for m in got[:-1]), "%s: a member that ends inside a row" % what
    return len(got)


ROW_OPTS = [dict(sam=True, blast=False), dict(sam=False, blast=True, cols="cigar qcov qstrand"), dict(sam=True, blast=True), dict(sam=True, blast=True, cols="qstrand cigar")]


def rows_key_body(e, slot, p, ix, db, what):
    """every option set of ROW_OPTS on the (index, part) of p -> the largest number of members a stream had"""
    lam, K, fr, fq = db
    most = 0
    for o in ROW_OPTS:
        kw = dict(o, lam=lam, K=K, full_ref=fr, full_read=fq)
        sam, blast = e.rows_part(slot, p, ix, **kw)
        sam_gz, blast_gz, plain_off = e.rows_part_gz(slot, p, ix, **kw)
        t = e.rows_times()
        assert t["d2h"] == 0 and (t["write"] > 0 or not (sam or blast)), t
        w = "%s, %s" % (what, o)
        assert plain_off == [0, len(sam), len(sam) + len(blast)], "%s: plain_off %s" % (w, plain_off)
        if not o["sam"]:
            assert sam_gz == b"" and sam == b""
        if not o["blast"]:
            assert blast_gz == b"" and blast == b""
        most = max(most, stream_check(e, sam, sam_gz, w + ": SAM"), stream_check(e, blast, blast_gz, w + ": BLAST"))
        assert len(sam_gz) + len(blast_gz) <= e.gzip_lines_bound(len(sam) + len(blast), 2)
        assert e.rows_part_gz(slot, p, ix, **kw)[:2] == (sam_gz, blast_gz), "%s: two calls, two outputs" % w
    return most


def pairwise_key_body(e, slot, p, ix, db, what):
    lam, K, fr, fq = db
    plain = e.pairwise_part(slot, p, ix, lam=lam, K=K, full_ref=fr, full_read=fq)
    gz, plain_bytes = e.pairwise_part_gz(slot, p, ix, lam=lam, K=K, full_ref=fr, full_read=fq)
    t = e.pairwise_times()
    assert t["d2h"] == 0 and (t["write"] > 0 or not plain), t
    assert plain_bytes == len(plain), "%s: plain_bytes %d, the sibling's text has %d" % (what, plain_bytes, len(plain))
    n = stream_check(e, plain, gz, what + ": pairwise")
    assert len(gz) <= e.gzip_lines_bound(len(plain), 1)
    assert e.pairwise_part_gz(slot, p, ix, lam=lam, K=K, full_ref=fr, full_read=fq) == (gz, plain_bytes), "%s: two calls, two outputs" % what
    return n


def crafted_body(n, fastq, pairwise=False):
    """the crafted state of helpers/rows.py: every key, every option set; at 1 025 reads the streams of key (0, 0) have several members"""
    from test_gpu_rows import crafted_engine
    e, reads, recs, reg = crafted_engine(n, fastq, seed=n)
    try:
        most = 0
        for key, ix in reg.items():
            p = smr.default_params()
            p.index_num, p.part = key
            body = pairwise_key_body if pairwise else rows_key_body
            most = max(most, body(e, 0, p, ix, rows.DB[key[0]], "%d reads, key %s" % (n, key)))
        assert most > 1 or n < 1025, "%d reads: one member at the most: the cuts were not exercised" % n
        assert e.export_records() == recs                             # no stored state changed
    finally:
        e.close()
        reads.free()


def golden_body(case="two_db_default"):
    """a golden workload with its stored records: each stream of either _gz call against its sibling, every member but the last a whole number
    of rows"""
    from test_gpu_pairwise import corrected_dbs
    from test_gpu_state_import import case_setup, engine
    cs = case_setup(case)
    data = open(golden.inputs(case)[1], "rb").read()
    recs = golden.records(case)
    e = engine()
    try:
        reads = e.upload_fastx(data, cs["slots"], view=True, keep=True)
        assert reads.count == len(recs)
        e.import_state(recs)
        dbs = corrected_dbs(cs)
        n_sam, most = 0, 0
        for j, (k, part, ix) in enumerate(cs["steps"]):
            e.upload_index(ix, j)
            p = cs["plist"][k]
            p.index_num, p.part = k, part
            most = max(most, rows_key_body(e, j, p, ix, dbs[k], "%s, key (%d, %d)" % (case, k, part)))
            most = max(most, pairwise_key_body(e, j, p, ix, dbs[k], "%s, key (%d, %d)" % (case, k, part)))
            n_sam += len(e.rows_part(j, p, ix)[0])
        print("%s: %d bytes of SAM rows, %d members in a stream at the most" % (case, n_sam, most))
        assert n_sam > 4096 and most > 1, "%s: %d bytes of SAM rows, %d members at the most: the comparison shows nothing" % (case, n_sam, most)
        reads.free()
    finally:
        e.close()


def _rows_call(e, slot, p, ix, o, buf, cap):
    gz_off, plain_off, need = (C.c_uint64 * 3)(9, 9, 9), (C.c_uint64 * 3)(9, 9, 9), C.c_uint64(9)
    rc = e.L.smr_rows_part_gz(e.h, slot, C.byref(p), ix.h, C.byref(o), buf.ctypes.data if buf is not None else None, cap, gz_off, plain_off, C.byref(need))
    return rc, list(gz_off), list(plain_off), need.value


def _pair_call(e, slot, p, ix, buf, cap, db=rows.DB[0]):
    plain, need = C.c_uint64(9), C.c_uint64(9)
    rc = e.L.smr_pairwise_part_gz(e.h, slot, C.byref(p), ix.h, db[0], db[1], db[2], db[3], buf.ctypes.data if buf is not None else None, cap, C.byref(plain), C.byref(need))
    return rc, plain.value, need.value


def _opts(sam=1, blast=1, cols="cigar qcov qstrand"):
    o = capi.RowsOpts()
    o.want_sam, o.want_blast, o.blast_cols = sam, blast, cols.encode()
    o.lam, o.K, o.full_ref_corr, o.full_read_corr = rows.DB[0]
    return o


def refusals_body():
    """the contract and the refusals of the plain calls, asked of the _gz calls; the messages name them; the context stays usable"""
    from test_gpu_rows import crafted_engine, syn_part
    ix, lens = syn_part()
    e, reads, recs, reg = crafted_engine(130, True, seed=9)
    p = smr.default_params()
    L = e.L

    def msg():
        return L.smr_last_error(e.h).decode()

    try:
        sam, blast = e.rows_part(0, p, ix, sam=True, blast=True, cols="cigar qcov qstrand", lam=rows.DB[0][0], K=rows.DB[0][1], full_ref=rows.DB[0][2], full_read=rows.DB[0][3])
        text = e.pairwise_part(0, p, ix, *rows.DB[0])

        def usable():
            rc, gz_off, plain_off, need = _rows_call(e, 0, p, ix, _opts(), big, len(big))
            assert rc == 0 and inflate(big[:gz_off[1]].tobytes()) == sam and inflate(big[gz_off[1]:need].tobytes()) == blast, "the context is not usable after a refusal"
            rc, plain, need = _pair_call(e, 0, p, ix, big, len(big))
            assert rc == 0 and plain == len(text) and inflate(big[:need].tobytes()) == text, "the context is not usable after a refusal"

        big = np.zeros(e.gzip_lines_bound(len(sam) + len(blast) + len(text), 2), dtype=np.uint8)
        # sizes only, one byte short, bytes to spare
        rc, gz_off, plain_off, need = _rows_call(e, 0, p, ix, _opts(), None, 0)
        assert rc == 0 and gz_off[0] == 0 and gz_off[2] == need and 0 < need < len(sam) + len(blast) and plain_off == [0, len(sam), len(sam) + len(blast)]
        buf = np.full(need + 64, 0x5A, dtype=np.uint8)
        rc, gz_off2, plain_off2, need2 = _rows_call(e, 0, p, ix, _opts(), buf, need - 1)
        assert rc == ERR_CAPACITY and "smr_rows_part_gz:" in msg() and (buf == 0x5A).all() and (gz_off2, plain_off2, need2) == (gz_off, plain_off, need)
        rc, gz_off2, plain_off2, need2 = _rows_call(e, 0, p, ix, _opts(), buf, need + 64)
        assert rc == 0 and (gz_off2, plain_off2, need2) == (gz_off, plain_off, need) and (buf[need:] == 0x5A).all()
        assert inflate(buf[:gz_off[1]].tobytes()) == sam and inflate(buf[gz_off[1]:need].tobytes()) == blast
        rc, plain, need = _pair_call(e, 0, p, ix, None, 0)
        assert rc == 0 and plain == len(text) and 0 < need < plain
        buf = np.full(need + 64, 0x5A, dtype=np.uint8)
        rc, plain2, need2 = _pair_call(e, 0, p, ix, buf, need - 1)
        assert rc == ERR_CAPACITY and "smr_pairwise_part_gz:" in msg() and (buf == 0x5A).all() and (plain2, need2) == (plain, need)
        rc, plain2, need2 = _pair_call(e, 0, p, ix, buf, need + 64)
        assert rc == 0 and (plain2, need2) == (plain, need) and (buf[need:] == 0x5A).all() and inflate(buf[:need].tobytes()) == text
        # no alignment of the key: nothing
        p.index_num, p.part = 3, 2
        assert _rows_call(e, 0, p, ix, _opts(), big, len(big)) == (0, [0, 0, 0], [0, 0, 0], 0)
        assert _pair_call(e, 0, p, ix, big, len(big)) == (0, 0, 0)
        p.index_num, p.part = 0, 0
        # the refusals of the arguments
        big[:] = 0x5A
        assert _rows_call(e, 0, p, ix, _opts(sam=0, blast=0), big, len(big))[0] == ERR_ARG and "smr_rows_part_gz:" in msg()
        assert _rows_call(e, 0, p, ix, _opts(cols="cigar qcov strand"), big, len(big))[0] == ERR_ARG and "smr_rows_part_gz:" in msg()
        assert _rows_call(e, 64, p, ix, _opts(), big, len(big))[0] == ERR_ARG and _pair_call(e, -1, p, ix, big, len(big))[0] == ERR_ARG
        o = _opts()
        g3, n1 = (C.c_uint64 * 3)(), C.c_uint64()
        assert L.smr_rows_part_gz(e.h, 0, C.byref(p), ix.h, C.byref(o), None, 0, None, g3, C.byref(n1)) == ERR_ARG
        assert L.smr_rows_part_gz(e.h, 0, C.byref(p), ix.h, C.byref(o), None, 0, g3, None, C.byref(n1)) == ERR_ARG
        assert L.smr_rows_part_gz(e.h, 0, C.byref(p), ix.h, C.byref(o), None, 0, g3, g3, None) == ERR_ARG
        assert L.smr_pairwise_part_gz(e.h, 0, C.byref(p), ix.h, 0.6, 0.3, 1, 1, None, 0, None, C.byref(n1)) == ERR_ARG
        assert L.smr_pairwise_part_gz(e.h, 0, C.byref(p), ix.h, 0.6, 0.3, 1, 1, None, 0, C.byref(n1), None) == ERR_ARG
        # `ix` of another part than the one in the slot
        other = smr.Index.build(golden.inputs("t9")[0], 18, 3072.0, 10000, 0)[0]
        assert _rows_call(e, 0, p, other, _opts(), big, len(big))[0] == ERR_ARG and "smr_rows_part_gz:" in msg() and "slot" in msg()
        assert _pair_call(e, 0, p, other, big, len(big))[0] == ERR_ARG and "smr_pairwise_part_gz:" in msg() and "slot" in msg()
        other.free()
        assert (big == 0x5A).all()
        usable()
        # a batch without kept text
        big[:] = 0x5A
        e.select_batch(1)
        plain_reads = smr.Reads.from_seqs([reads.record_text(i)[1] for i in range(reads.count)])
        e.upload_reads(plain_reads, 6)
        e.import_state(recs)
        assert _rows_call(e, 0, p, ix, _opts(), big, len(big))[0] == ERR_STATE and "SMR_FASTX_KEEP" in msg() and "smr_rows_part_gz:" in msg()
        assert _pair_call(e, 0, p, ix, big, len(big))[0] == ERR_STATE and "SMR_FASTX_KEEP" in msg() and "smr_pairwise_part_gz:" in msg()
        assert (big == 0x5A).all()
        plain_reads.free()
        e.select_batch(0)
        usable()
        assert e.rows_part(0, p, ix, sam=True)[0] == sam                         # the sibling still gives its stream
        assert e.export_records() == recs
    finally:
        e.close()
        reads.free()
