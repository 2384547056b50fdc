"""TEST INFRASTRUCTURE: a plain-Python inflate that says where the blocks and members of a gzip file begin -- the model the device decoder's task
starts are compared with -- and a small DEFLATE writer for streams zlib never emits (a distance of 32 768, a reference in front of a member's
first byte).  The model is no yardstick of its own: model() asserts that its bytes are zlib's for every blob it is asked about."""
import zlib

ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def canonical(lens):
    """code lengths -> {symbol: (code, length)} (RFC 1951, 3.2.2)"""
    out, code = {}, 0
    for bits in range(1, 16):
        for s, l in enumerate(lens):
            if l == bits:
                out[s] = (code, bits)
                code += 1
        code <<= 1
    return out


def _table(lens):
    """-> (list indexed by the next `top` bits of the stream: symbol << 4 | length, or -1; top)"""
    top = max(lens) if any(lens) else 1
    tab = [-1] * (1 << top)
    for s, (code, l) in canonical(lens).items():
        rev = int(format(code, "0%db" % l)[::-1], 2)
        for k in range(rev, 1 << top, 1 << l):
            tab[k] = (s << 4) | l
    return tab, top


_FIXED = None


def _fixed():
    global _FIXED
    if _FIXED is None:
        _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8), _table([5] * 32))
    return _FIXED


class _Bits:
    def __init__(self, data, byte):
        self.d, self.at, self.buf, self.cnt = data, byte, 0, 0

    def pos(self):
        return self.at * 8 - self.cnt

    def need(self, n):
        while self.cnt < n:
            self.buf |= int.from_bytes(self.d[self.at:self.at + 8].ljust(8, b"\0"), "little") << self.cnt
            self.at += 8
            self.cnt += 64

    def take(self, n):
        self.need(n)
        v = self.buf & ((1 << n) - 1)
        self.buf >>= n
        self.cnt -= n
        return v

    def seek_byte(self, byte):
        self.at, self.buf, self.cnt = byte, 0, 0

    def sym(self, tab, top):
        self.need(top)
        e = tab[self.buf & ((1 << top) - 1)]
        assert e >= 0, "an unused code"
        self.buf >>= e & 15
        self.cnt -= e & 15
        return e >> 4


def skip_header(blob, at):
    """the gzip member header at byte `at` -> the first byte behind it"""
    assert blob[at:at + 3] == b"\x1f\x8b\x08" and not blob[at + 3] & 0xE0, "no member header at byte %d" % at
    flg, p = blob[at + 3], at + 10
    if flg & 4:
        p += 2 + blob[p] + (blob[p + 1] << 8)
    for f in (8, 16):
        if flg & f:
            p = blob.index(b"\0", p) + 1
    if flg & 2:
        p += 2
    return p


def inflate(blob):
    """-> (plain bytes, blocks [(bit offset of the block header, BTYPE, BFINAL, member)], members [(header byte, first data byte, byte behind the trailer)])"""
    out, blocks, members = bytearray(), [], []
    at = 0
    while at < len(blob):
        data = skip_header(blob, at)
        b = _Bits(blob, data)
        begin = len(out)
        while True:
            blocks.append((b.pos(), None, None, len(members)))
            final, btype = b.take(1), b.take(2)
            blocks[-1] = (blocks[-1][0], btype, final, len(members))
            if btype == 0:
                byte = (b.pos() + 7) // 8
                n = blob[byte] | (blob[byte + 1] << 8)
                assert n == (blob[byte + 2] | (blob[byte + 3] << 8)) ^ 0xFFFF
                out += blob[byte + 4:byte + 4 + n]
                b.seek_byte(byte + 4 + n)
            else:
                assert btype in (1, 2)
                if btype == 1:
                    (lt, ltop), (dt, dtop) = _fixed()
                else:
                    hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                    cl = [0] * 19
                    for k in range(hclen):
                        cl[ORDER[k]] = b.take(3)
                    ct, ctop = _table(cl)
                    lens = []
                    while len(lens) < hlit + hdist:
                        s = b.sym(ct, ctop)
                        if s < 16:
                            lens.append(s)
                        elif s == 16:
                            lens += [lens[-1]] * (3 + b.take(2))
                        elif s == 17:
                            lens += [0] * (3 + b.take(3))
                        else:
                            lens += [0] * (11 + b.take(7))
                    assert len(lens) == hlit + hdist
                    (lt, ltop), (dt, dtop) = _table(lens[:hlit]), _table(lens[hlit:])
                while True:
                    s = b.sym(lt, ltop)
                    if s < 256:
                        out.append(s)
                    elif s == 256:
                        break
                    else:
                        n = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
                        d = b.sym(dt, dtop)
                        dist = DIST_BASE[d] + b.take(DIST_EXTRA[d])
                        assert dist <= len(out) - begin, "a distance too far back"
                        if dist >= n:
                            out += out[len(out) - dist:len(out) - dist + n]
                        else:
                            for _ in range(n):
                                out.append(out[-dist])
            if final:
                break
        end = (b.pos() + 7) // 8 + 8
        members.append((at, data, end))
        at = end
    return bytes(out), blocks, members


_models = {}


def model(blob):
    """inflate(blob), asserted to give zlib's bytes; cached per blob"""
    if blob not in _models:
        out, blocks, members = inflate(blob)
        want, rest = bytearray(), blob
        while rest:
            d = zlib.decompressobj(31)
            want += d.decompress(rest) + d.flush()
            assert d.eof
            rest = d.unused_data
        assert out == bytes(want), "the model's bytes are not zlib's"
        _models[blob] = (out, blocks, members)
    return _models[blob]


def task_starts(blob):
    """where a decoder that starts a task at every candidate must begin: [(bit, at a member header)] -- the member headers and the non-final
    dynamic-Huffman blocks, in file order"""
    _, blocks, members = model(blob)
    s = [(m[0] * 8, True) for m in members] + [(bit, False) for bit, btype, final, _ in blocks if btype == 2 and not final]
    return sorted(s)


# ---------------------------------------------------------------------------------------------------- a DEFLATE writer
class Writer:
    """bits of a raw DEFLATE stream, least significant first"""

    def __init__(self, head=b""):
        self.out, self.buf, self.cnt = bytearray(head), 0, 0

    def bits(self, v, n):
        self.buf |= v << self.cnt
        self.cnt += n
        while self.cnt >= 8:
            self.out.append(self.buf & 0xFF)
            self.buf >>= 8
            self.cnt -= 8

    def code(self, c):
        code, l = c
        self.bits(int(format(code, "0%db" % l)[::-1], 2), l)

    def align(self):
        if self.cnt:
            self.bits(0, 8 - self.cnt)

    def raw(self, data):
        """byte-aligned DEFLATE data as zlib wrote it (up to a sync flush)"""
        assert self.cnt == 0
        self.out += data

    def stored(self, payload, final=False):
        assert len(payload) <= 65535
        self.bits(final, 1)
        self.bits(0, 2)
        self.align()
        self.out += len(payload).to_bytes(2, "little") + (len(payload) ^ 0xFFFF).to_bytes(2, "little") + payload

    def end_fixed(self):
        """a final fixed-Huffman block that holds nothing"""
        self.bits(1, 1)
        self.bits(1, 2)
        self.bits(0, 7)
        self.align()

    def dynamic(self, tokens, final=False):
        """a dynamic-Huffman block of the tokens (a literal byte, or (length, distance)).  Every used symbol gets the same length: the used
        symbols are topped up to a power of two, so both codes are complete; the code lengths are sent one by one under a code-length code
        of sixteen 4-bit codes."""
        def sym_of(v, base):
            return max(i for i, b in enumerate(base) if b <= v)

        lit_used, dist_used = {256}, set()
        for t in tokens:
            if isinstance(t, tuple):
                lit_used.add(257 + sym_of(t[0], LEN_BASE))
                dist_used.add(sym_of(t[1], DIST_BASE))
            else:
                lit_used.add(t)

        def lengths(used, n, least):
            want = least
            while want < len(used):
                want *= 2
            fill = [s for s in range(n) if s not in used]
            used = sorted(used) + fill[:want - len(used)]
            assert len(used) == want
            bits = want.bit_length() - 1
            return [bits if s in set(used) else 0 for s in range(n)]

        ll, dl = lengths(lit_used, 286, 2), lengths(dist_used, 30, 2)
        lc, dc = canonical(ll), canonical(dl)
        self.bits(final, 1)
        self.bits(2, 2)
        self.bits(286 - 257, 5)
        self.bits(30 - 1, 5)
        self.bits(19 - 4, 4)
        for s in ORDER:
            self.bits(4 if s < 16 else 0, 3)
        for l in ll + dl:
            self.code((l, 4))
        for t in tokens:
            if isinstance(t, tuple):
                s = sym_of(t[0], LEN_BASE)
                self.code(lc[257 + s])
                self.bits(t[0] - LEN_BASE[s], LEN_EXTRA[s])
                d = sym_of(t[1], DIST_BASE)
                self.code(dc[d])
                self.bits(t[1] - DIST_BASE[d], DIST_EXTRA[d])
            else:
                self.code(lc[t])
        self.code(lc[256])

    def bytes(self):
        self.align()
        return bytes(self.out)


def member(raw, plain, header=b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\xff"):
    """a gzip member around raw DEFLATE data that inflates to plain"""
    return header + raw + zlib.crc32(plain).to_bytes(4, "little") + (len(plain) & 0xFFFFFFFF).to_bytes(4, "little")


def raw_inflate(raw):
    d = zlib.decompressobj(-15)
    out = d.decompress(raw) + d.flush()
    assert d.eof and not d.unused_data
    return out
