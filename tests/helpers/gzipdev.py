"""TEST INFRASTRUCTURE: the bodies of the device gzip tests (test_gpu_gzip.py runs them on the GPU, test_emu_gzip.py on the kernel emulator).

Every yardstick is Python's gzip / zlib -- the reference's own compressor -- or the host model of helpers/fxsplit.py; never the code under
test.  A device output is accepted when zlib inflates it to the input, member by member: that checks the DEFLATE data, the distances (zlib
refuses one that is too far), each member's CRC-32 and ISIZE."""
import ctypes as C
import gzip
import os
import random
import zlib

import numpy as np

import sortmerna_amd as smr
from sortmerna_amd import capi

from . import fxsplit, paths

ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -4, -5
AMPLICON = os.path.join(paths.GOLDEN, "config2", "set2_environmental_study_550_amplicon.fasta.gz")


def _lib():
    return capi._lib or capi.load()                     # (the emulator's library while helpers.emu.active() holds)


def chunk():
    return int(_lib().smr_gzip_chunk())


# ------------------------------------------------------------------------------------------------ yardsticks
def members(blob):
    """the gzip members of blob, each inflated by zlib (header, CRC-32 and ISIZE checked) -> [plain bytes]"""
    out = []
    while blob:
        d = zlib.decompressobj(31)
        plain = d.decompress(blob) + d.flush()
        assert d.eof, "a member that does not end"
        out.append(plain)
        blob = d.unused_data
    return out


def bound_formula(n, c):
    """per member 18 + plain + 5 * ceil(plain / 65 535), over the chunks of one stream of n bytes"""
    return sum(18 + p + 5 * ((p + 65534) // 65535) for p in (min(c, n - at) for at in range(0, n, c)))


def check(data, out, what):
    """out is data as gzip members of one chunk each, within the bound"""
    c = chunk()
    n_chunks = (len(data) + c - 1) // c
    if not data:
        assert out == b"", "%s: an empty stream produces bytes" % what
        return
    assert gzip.decompress(out) == data, "%s: does not inflate to the input" % what
    got = members(out)
    assert len(got) == n_chunks, "%s: %d members for %d chunks" % (what, len(got), n_chunks)
    for k, m in enumerate(got):
        assert m == data[k * c:(k + 1) * c], "%s: member %d is not its chunk" % (what, k)
    assert out[:10] == b"\x1f\x8b\x08\x00\x00\x00\x00\x00" + out[8:10], "%s: a header with a name, flags or an mtime" % what
    bound = int(_lib().smr_gzip_bound(len(data), n_chunks))
    assert bound == bound_formula(len(data), c), "%s: smr_gzip_bound(%d, %d) = %d" % (what, len(data), n_chunks, bound)
    assert len(out) <= bound, "%s: %d bytes, the bound is %d" % (what, len(out), bound)


def seeded(n, seed):
    return random.Random(seed).randbytes(n)


def texty(n, seed):
    """n bytes that look like reads: lines of letters with repeats nearby and far away"""
    rng = random.Random(seed)
    lines = [bytes(rng.choice(b"ACGT") for _ in range(40 + rng.randrange(60))) for _ in range(50)]
    out = bytearray()
    k = 0
    while len(out) < n:
        out += b"@read%d/%d\n" % (k, seed) + lines[rng.randrange(50)] + b"\n+\n" + bytes(33 + rng.randrange(8) for _ in range(50)) + b"\n"
        k += 1
    return bytes(out[:n])


_inputs = {}
INPUT_NAMES = ["0 bytes", "1 bytes", "2 bytes", "3 bytes", "4 bytes", "C - 1 bytes", "C bytes", "C + 1 bytes", "2 C bytes", "2 C + 1 bytes", "all one byte",
               "a period of 258", "a period of 259", "FASTQ text", "one pair of bytes", "all 256 byte values once"]


def inputs():
    """name -> bytes: the inputs of the round-trip test (each a stream of its own)"""
    if _inputs:
        return _inputs
    from test_gpu_fastx_device import scan_text
    c = chunk()
    for name, n in zip(INPUT_NAMES, (0, 1, 2, 3, 4, c - 1, c, c + 1, 2 * c, 2 * c + 1)):
        _inputs[name] = texty(n, n)
    _inputs["all one byte"] = b"G" * (c + 777)
    _inputs["a period of 258"] = (seeded(258, 1) * 80)[:20000]
    _inputs["a period of 259"] = (seeded(259, 2) * 80)[:20000]
    _inputs["FASTQ text"] = scan_text(True, 1025)
    _inputs["one pair of bytes"] = b"AB" * (c // 2)
    _inputs["all 256 byte values once"] = bytes(range(256))
    assert list(_inputs) == INPUT_NAMES
    return _inputs


def far_inputs():
    """a repeat at distance 32 768 (the farthest DEFLATE can name) and one at 32 769: random bytes, then their first 1 000 again"""
    return {"a repeat at distance 32768": seeded(32768, 3) + seeded(32768, 3)[:1000], "a repeat at distance 32769": seeded(32769, 4) + seeded(32769, 4)[:1000]}


# ------------------------------------------------------------------------------------------------ 1. round trip and framing; 3. the bound
def round_trip_body(names=None):
    e = smr.Engine(0)
    try:
        for name in (names or INPUT_NAMES):
            data = inputs()[name]
            check(data, e.gzip_batch([data])[0], name)
    finally:
        e.close()


def far_body():
    e = smr.Engine(0)
    try:
        for name, data in far_inputs().items():
            out = e.gzip_batch([data])[0]
            check(data, out, name)
        near = far_inputs()["a repeat at distance 32768"]
        assert len(e.gzip_batch([near])[0]) < len(near) - 500, "the repeat at distance 32 768 was not found"
    finally:
        e.close()


def eight_streams():
    """empty streams first, last and in between; the others begin at every byte phase mod 4"""
    c = chunk()
    s = [b"", texty(1, 11), texty(c + 2, 12), b"", texty(4, 13), texty(7, 14), seeded(300, 15), b""]
    starts = {sum(len(x) for x in s[:k]) & 3 for k in range(8) if s[k]}
    assert starts == {0, 1, 2, 3}, starts
    return s


def eight_streams_body():
    e = smr.Engine(0)
    try:
        s = eight_streams()
        out = e.gzip_batch(s)
        for k in range(8):
            check(s[k], out[k], "stream %d of eight" % k)
    finally:
        e.close()


def incompressible_body():
    e = smr.Engine(0)
    c = chunk()
    try:
        for n in (1, 65535, 65536, c, 2 * c + 1):
            data = seeded(n, n)
            out = e.gzip_batch([data])[0]
            check(data, out, "%d random bytes" % n)
            if n >= 65535:
                assert len(out) >= n, "%d random bytes became %d" % (n, len(out))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 2. code limits
def huffman_depth(freqs):
    """the longest code of an unlimited Huffman code over the non-zero frequencies"""
    import heapq
    h = [(f, 0, i) for i, f in enumerate(freqs) if f]
    if len(h) < 2:
        return len(h)
    heapq.heapify(h)
    k = len(freqs)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], max(a[1], b[1]) + 1, k))
        k += 1
    return h[0][1]


def fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def fibonacci_chunk():
    c = chunk()
    f = fib(24 if sum(fib(24)) <= c else 20)
    data = bytearray()
    for i, k in enumerate(f):
        data += bytes([65 + i]) * k
    random.Random(24).shuffle(data)
    return bytes(data), f


class Bits:
    def __init__(self, data, at):
        self.d, self.p = data, at * 8

    def take(self, n):
        v = 0
        for k in range(n):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << k
            self.p += 1
        return v


def canonical_decoder(lens):
    """code lengths -> {(length, code): symbol} (RFC 1951, 3.2.2)"""
    code, table = 0, {}
    for bits in range(1, 16):
        for s, l in enumerate(lens):
            if l == bits:
                table[(bits, code)] = s
                code += 1
        code <<= 1
    return table


def dynamic_header(member):
    """the first block of a gzip member, which must be a dynamic-Huffman block -> (literal/length lengths, distance lengths, the code-length
    symbols as they were sent, the code-length code's lengths)"""
    b = Bits(member, 10)
    b.take(1)
    assert b.take(2) == 2, "not a dynamic-Huffman block"
    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
    cl = [0] * 19
    for k in range(hclen):
        cl[[16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15][k]] = b.take(3)
    dec = canonical_decoder(cl)
    lens, sent = [], []
    while len(lens) < hlit + hdist:
        code, n = 0, 0
        while (n, code) not in dec:
            code = (code << 1) | b.take(1)
            n += 1
            assert n <= 7
        s = dec[(n, code)]
        sent.append(s)
        if s < 16:
            lens.append(s)
        elif s == 16:
            lens += [lens[-1]] * (3 + b.take(2))
        elif s == 17:
            lens += [0] * (3 + b.take(3))
        else:
            lens += [0] * (11 + b.take(7))
    return lens[:hlit], lens[hlit:], sent, cl


def literal_limit_body():
    data, f = fibonacci_chunk()
    assert len(data) in (121392, 17710) and huffman_depth(f) > 15, (len(data), huffman_depth(f))
    e = smr.Engine(0)
    try:
        out = e.gzip_batch([data])[0]
        check(data, out, "Fibonacci frequencies over %d symbols" % len(f))
        lit, dist, _, _ = dynamic_header(out)
        print("Fibonacci chunk: %d bytes -> %d, longest literal/length code %d, longest distance code %d" % (len(data), len(out), max(lit), max(dist)))
        assert max(lit) <= 15 and max(dist) <= 15
    finally:
        e.close()


def de_bruijn_pairs(k):
    """a sequence over k symbols in which every ordered pair of neighbours occurs once (the de Bruijn sequence B(k, 2), Lyndon words)"""
    a, seq = [0] * (2 * 2), []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq


def no_repeat_chunk(freqs, n_fill):
    """bytes 0 .. len(freqs) - 1 with the given frequencies at the even places, n_fill filler bytes at the odd ones, the fillers in an order
    in which no pair of neighbouring fillers occurs twice: no four bytes of the chunk occur twice, so LZ77 with matches of four bytes or more
    finds nothing and the literal frequencies reach the Huffman stage as they are"""
    body = bytearray()
    for i, f in enumerate(freqs):
        body += bytes([i]) * f
    random.Random(len(freqs)).shuffle(body)
    assert len(body) <= n_fill * n_fill and len(freqs) + n_fill <= 256
    fill = de_bruijn_pairs(n_fill)[:len(body)]
    out = bytearray(2 * len(body))
    out[0::2] = body
    out[1::2] = bytes(len(freqs) + x for x in fill)
    grams = {bytes(out[i:i + 4]) for i in range(len(out) - 3)}
    assert len(grams) == len(out) - 3
    return bytes(out)


def code_length_chunk():
    """n_L bytes meant to get L bits (frequency 2^(13 - L) of 4 096 even places), n_L growing like the Fibonacci numbers with L, between 64
    fillers of 64 places each (7 bits): the lengths that are sent are then as skewed as the bytes of fibonacci_chunk"""
    counts = {2: 1, 3: 1, 5: 2, 7: 2, 8: 3, 9: 5, 10: 8, 11: 13, 12: 21, 13: 50}       # (with the fillers the lengths fill the code space: Kraft sum 1)
    freqs = [1 << (13 - L) for L, n in counts.items() for _ in range(n)]
    assert sum(freqs) == 4096
    return no_repeat_chunk(freqs, 64)


def code_length_limit_body():
    data = code_length_chunk()
    assert len(data) <= chunk()
    e = smr.Engine(0)
    try:
        out = e.gzip_batch([data])[0]
        check(data, out, "a skewed code-length alphabet")
        lit, dist, sent, cl = dynamic_header(out)
        freq = [sent.count(s) for s in range(19)]
        print("code-length symbols sent:", freq, "unlimited depth", huffman_depth(freq), "lengths used", cl)
        assert huffman_depth(freq) > 7, "the chunk does not ask for a code-length code of more than 7 bits: %s" % freq
        assert max(cl) <= 7
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 4. it compresses, and it matches
def fasta_body():
    rng = random.Random(1000)
    data = b"".join(b">r%d\n%s\n" % (i, bytes(rng.choice(b"ACGT") for _ in range(150))) for i in range(1000))
    assert len(data) == 156890
    e = smr.Engine(0)
    try:
        out = e.gzip_batch([data])[0]
        check(data, out, "1 000 FASTA records")
        print("1 000 FASTA records: %d -> %d bytes (%.3f of plain)" % (len(data), len(out), len(out) / len(data)))
        assert len(out) < 0.5 * len(data)
    finally:
        e.close()


def zsize(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    z = zlib.compressobj(level, zlib.DEFLATED, 31, 8, strategy)
    return len(z.compress(data) + z.flush())


def amplicon_body(n_bytes):
    data = gzip.open(AMPLICON, "rb").read(n_bytes)
    assert len(data) == n_bytes
    e = smr.Engine(0)
    try:
        out = e.gzip_batch([data])[0]
        check(data, out, "amplicon reads")
        huff, l1, l6 = zsize(data, 6, zlib.Z_HUFFMAN_ONLY), zsize(data, 1), zsize(data, 6)
        print("amplicon reads, %d bytes: device %.3f of plain; zlib Huffman only %.3f, level 1 %.3f, level 6 %.3f; device / level 1 = %.2f, device / level 6 = %.2f" % (
            n_bytes, len(out) / n_bytes, huff / n_bytes, l1 / n_bytes, l6 / n_bytes, len(out) / l1, len(out) / l6))
        assert len(out) < huff, "the device's %d bytes are no smaller than Huffman coding alone (%d)" % (len(out), huff)
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 5. determinism
def determinism_body():
    e, e2 = smr.Engine(0), smr.Engine(0)
    try:
        s = eight_streams()
        first = e.gzip_batch(s)
        assert e.gzip_batch(s) == first, "two calls, two outputs"
        assert e2.gzip_batch(s) == first, "two contexts, two outputs"
        for k in (2, 6):
            assert e.gzip_batch([s[k]])[0] == first[k], "stream %d alone differs from the same bytes among eight" % k
        t = inputs()["FASTQ text"]
        assert e.gzip_batch([b"x", t, b""])[1] == e.gzip_batch([t])[0]
    finally:
        e.close()
        e2.close()


def batch_contract_body():
    """smr_gzip_batch: sizes only, one byte short, spare bytes, NULL arguments"""
    e = smr.Engine(0)
    L = e.L
    try:
        data = inputs()["FASTQ text"]
        plain = np.frombuffer(data, dtype=np.uint8)
        off = (C.c_uint64 * 2)(0, len(data))
        gz_off, need = (C.c_uint64 * 2)(7, 7), C.c_uint64(7)
        assert L.smr_gzip_batch(e.h, plain.ctypes.data, off, 1, None, 0, gz_off, C.byref(need)) == 0
        total = need.value
        assert list(gz_off) == [0, total] and 0 < total < len(data)
        buf = np.full(total + 64, 0xA5, dtype=np.uint8)
        assert L.smr_gzip_batch(e.h, plain.ctypes.data, off, 1, buf.ctypes.data, total - 1, gz_off, C.byref(need)) == ERR_CAPACITY
        assert need.value == total and list(gz_off) == [0, total] and (buf == 0xA5).all() and b"smr_gzip_batch" in L.smr_last_error(e.h)
        assert L.smr_gzip_batch(e.h, plain.ctypes.data, off, 1, buf.ctypes.data, total + 64, gz_off, C.byref(need)) == 0
        assert need.value == total and (buf[total:] == 0xA5).all()
        check(data, buf[:total].tobytes(), "after a refusal")
        assert L.smr_gzip_batch(e.h, plain.ctypes.data, None, 1, None, 0, gz_off, C.byref(need)) == ERR_ARG
        assert L.smr_gzip_batch(e.h, plain.ctypes.data, off, 1, None, 0, None, C.byref(need)) == ERR_ARG
        assert L.smr_gzip_batch(e.h, plain.ctypes.data, off, 1, None, 0, gz_off, None) == ERR_ARG
        assert L.smr_gzip_batch(e.h, plain.ctypes.data, (C.c_uint64 * 2)(5, 4), 1, None, 0, gz_off, C.byref(need)) == ERR_ARG
        ms = e.gzip_times()
        assert set(ms) == {"match", "codes", "encode", "compact", "d2h"}
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 6. smr_fastx_split_gz / smr_fastx_denovo_gz
def inflate(blob):
    return gzip.decompress(blob) if blob else b""


def _host_reads(data, tmp_path, name):
    path = os.path.join(str(tmp_path), name)
    with open(path, "wb") as f:
        f.write(data)
    return smr.Reads.from_fastx_text(path)


def split_gz_equals(e, reads, hits, what, **opts):
    """stream k of the _gz call inflates to the sibling's stream k and to the host model's; plain_off is the sibling's off"""
    kw = {k: v for k, v in opts.items()}
    gz, plain_off = e.fastx_split_gz(hit=hits, **kw)
    sib = e.fastx_split(hit=hits, **kw)
    want = fxsplit.expected_streams(reads, hits, opts)
    at = [0]
    for k in range(8):
        assert inflate(gz[k]) == sib[k] == want[k], "%s: stream %d" % (what, k)
        assert bool(gz[k]) == bool(want[k]), "%s: stream %d is empty and has bytes" % (what, k)
        check(want[k], gz[k], "%s: stream %d" % (what, k))
        at.append(at[-1] + len(sib[k]))
    assert plain_off == at, "%s: plain_off %s, the sibling's %s" % (what, plain_off, at)


def split_gz_body(n_rec, tmp_path):
    from test_gpu_fastx_device import scan_text
    e = smr.Engine(0)
    try:
        data = scan_text(True, n_rec)
        reads = _host_reads(data, tmp_path, "reads.fq")
        e.upload_fastx(data, 1, view=True, keep=True).free()
        rng = random.Random(n_rec)
        hits = [rng.randrange(2) for _ in range(n_rec)]
        try:
            split_gz_equals(e, reads, hits, "%d records" % n_rec)
            split_gz_equals(e, reads, [0] * n_rec, "%d records, no hit" % n_rec)
            split_gz_equals(e, reads, [1] * n_rec, "%d records, all hits" % n_rec)
            if n_rec % 2 == 0:
                split_gz_equals(e, reads, hits, "%d records, interleaved, four files" % n_rec, layout=1, out2=True, sout=True)
        finally:
            reads.free()
    finally:
        e.close()


def split_gz_two_batches_body(tmp_path):
    from test_gpu_fastx_device import scan_text
    e = smr.Engine(0)
    try:
        d1, d2 = scan_text(True, 64), scan_text(True, 64).replace(b"@", b"@m")
        r1, r2 = _host_reads(d1, tmp_path, "m1.fq"), _host_reads(d2, tmp_path, "m2.fq")
        e.upload_fastx(d1, 1, view=True, keep=True).free()
        e.upload_fastx(d2, 1, batch=1, view=True, keep=True).free()
        rng = random.Random(2)
        hits = [rng.randrange(2) for _ in range(128)]
        try:
            for o in (dict(), dict(out2=True, sout=True), dict(paired_in=True)):
                gz, plain_off = e.fastx_split_gz(layout=2, mates=1, hit=hits, **o)
                sib = e.fastx_split(layout=2, mates=1, hit=hits, **o)
                want = fxsplit.expected_streams((r1, r2), hits, dict(layout=2, **o))
                for k in range(8):
                    assert inflate(gz[k]) == sib[k] == want[k], "two batches, %s: stream %d" % (fxsplit.opts_id(o), k)
                assert plain_off == [sum(len(x) for x in sib[:k]) for k in range(9)]
        finally:
            r1.free()
            r2.free()
    finally:
        e.close()


def denovo_gz_body(tmp_path, fastq):
    """the routing cases of helpers.otu_device.routing_body with a dn array: the _gz call against its sibling"""
    from . import otu_device as od
    e = smr.Engine(0)
    try:
        e.upload_fastx(od.routing_text(fastq, 6, "r"), 1, view=True, keep=True).free()
        e.select_batch(1)
        e.upload_fastx(od.routing_text(fastq, 3, "m"), 1, view=True, keep=True).free()
        e.select_batch(2)
        e.upload_fastx(od.routing_text(fastq, 3, "r"), 1, view=True, keep=True).free()
        n_case = 0
        for shift in range(4):
            combos = [(((shift + j) % 4) & 1, ((shift + j) % 4) >> 1) for j in range(3)]
            for o in fxsplit.VALID_OPTS:
                for layout in (0, 1, 2):
                    dn = [c[0] for c in combos] + [c[1] for c in combos] if layout == 2 else [combos[i // 2][i % 2] for i in range(6)]
                    e.select_batch(2 if layout == 2 else 0)
                    kw = dict(layout=layout, mates=1 if layout == 2 else None, dn=dn, **(o if layout else {}))
                    sib = e.fastx_denovo(**kw)
                    gz, plain_off = e.fastx_denovo_gz(**kw)
                    what = "dn %s, %s, layout %d" % (dn, fxsplit.opts_id(o), layout)
                    assert [inflate(x) for x in gz] == sib, what
                    assert [bool(x) for x in gz] == [bool(x) for x in sib], what
                    assert plain_off == [sum(len(x) for x in sib[:k]) for k in range(5)], what
                    n_case += 1
        assert n_case == 4 * 8 * 3
        e.select_batch(0)
        assert e.fastx_denovo_gz()[0] == [b""] * 4                   # without the override and without the pass: no de novo read
    finally:
        e.close()


def guards_gz_body(tmp_path):
    """what test_gpu_fastx_split.guards_body asks of the sibling, asked of the _gz calls"""
    from test_gpu_fastx_device import scan_text
    e = smr.Engine(0)
    L = e.L
    try:
        data = scan_text(True, 65)
        gz_off, plain_off, need = (C.c_uint64 * 9)(), (C.c_uint64 * 9)(), C.c_uint64()

        def split(layout=0, mates=-1, buf=None, cap=0, fn="smr_fastx_split_gz", **kw):
            o = capi.FxSplitOpts(layout, kw.get("paired_in", 0), kw.get("paired_out", 0), 0, 0, 1, 1)
            return getattr(L, fn)(e.h, mates, C.byref(o), None, buf, cap, gz_off, plain_off, C.byref(need))

        def usable():
            gz, _ = e.fastx_split_gz(hit=hits)
            assert [inflate(x) for x in gz] == want, "the context is not usable after a refusal"

        # no kept text
        e.upload_fastx(data).free()
        for fn in ("smr_fastx_split_gz", "smr_fastx_denovo_gz"):
            assert split(fn=fn) == ERR_STATE and b"SMR_FASTX_KEEP" in L.smr_last_error(e.h) and fn.encode() + b":" in L.smr_last_error(e.h)
        reads = _host_reads(data, tmp_path, "reads.fq")
        e.upload_fastx(data, 1, view=True, keep=True).free()
        hits = [i % 3 == 0 for i in range(reads.count)]
        want = fxsplit.expected_streams(reads, hits, {})
        usable()
        # sizes only, one byte short, 64 bytes to spare
        assert split() == 0
        total = need.value
        offs = list(gz_off)
        plain_total = len(fxsplit.expected_streams(reads, [0] * reads.count, {})[4])
        assert 0 < total < plain_total and offs == [0, 0, 0, 0, 0, total, total, total, total] and list(plain_off) == [0, 0, 0, 0, 0] + [plain_total] * 4
        buf = np.full(total + 64, 0xA5, dtype=np.uint8)
        need.value = 0
        assert split(buf=buf.ctypes.data, cap=total - 1) == ERR_CAPACITY and b"smr_fastx_split_gz" in L.smr_last_error(e.h)
        assert need.value == total and list(gz_off) == offs and list(plain_off)[8] == plain_total and (buf == 0xA5).all()
        usable()
        assert split(buf=buf.ctypes.data, cap=total + 64) == 0
        assert need.value == total and (buf[total:] == 0xA5).all() and inflate(buf[:total].tobytes()) == fxsplit.expected_streams(reads, [0] * reads.count, {})[4]
        first = buf[:total].tobytes()
        buf[:] = 0xA5
        assert split(buf=buf.ctypes.data, cap=total) == 0 and buf[:total].tobytes() == first and (buf[total:] == 0xA5).all()      # repeated: the same bytes
        # bad layouts and option sets, NULL arguments
        assert split(layout=1) == ERR_ARG                                       # 65 reads
        usable()
        assert split(layout=2, mates=0) == ERR_ARG                              # the selected batch
        usable()
        e.upload_fastx(scan_text(True, 64), 1, batch=1, view=True, keep=True).free()
        assert split(layout=2, mates=1) == ERR_ARG                              # 65 reads, 64 mates
        usable()
        assert split(layout=3) == ERR_ARG and split(layout=3, fn="smr_fastx_denovo_gz") == ERR_ARG
        o = capi.FxSplitOpts(0, 0, 0, 0, 0, 1, 1)
        for fn in ("smr_fastx_split_gz", "smr_fastx_denovo_gz"):
            f = getattr(L, fn)
            assert f(e.h, -1, None, None, None, 0, gz_off, plain_off, C.byref(need)) == ERR_ARG
            assert f(e.h, -1, C.byref(o), None, None, 0, None, plain_off, C.byref(need)) == ERR_ARG
            assert f(e.h, -1, C.byref(o), None, None, 0, gz_off, None, C.byref(need)) == ERR_ARG
            assert f(e.h, -1, C.byref(o), None, None, 0, gz_off, plain_off, None) == ERR_ARG
            assert f(None, -1, C.byref(o), None, None, 0, gz_off, plain_off, C.byref(need)) == ERR_ARG
        e.upload_fastx(scan_text(True, 64), 1, view=True, keep=True).free()
        assert split(layout=1, paired_in=1, paired_out=1) == ERR_ARG and split(layout=2, mates=1, paired_in=1, paired_out=1) == ERR_ARG
        e.upload_fastx(scan_text(False, 64), 1, batch=1, view=True, keep=True).free()
        assert split(layout=2, mates=1) == ERR_ARG                              # FASTQ reads, FASTA mates
        e.upload_fastx(data, 1, view=True, keep=True).free()
        usable()
        assert e.fastx_split(hit=hits) == want                                  # the sibling still gives its streams
        reads.free()
    finally:
        e.close()
