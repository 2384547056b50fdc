"""CPU: the report side of gzip on the device -- smr_report_add_fastx_gz / smr_report_add_denovo_gz append gzip members made elsewhere to the
open .gz files as they are.  The members here are Python's gzip.compress; the files are read back with Python's gzip, which inflates a
multi-member file the way any downstream tool has to."""
import ctypes as C
import gzip
import os

from sortmerna_amd import report

ERR_ARG = -1


def _open(d, **kw):
    os.makedirs(str(d), exist_ok=True)
    return report.Report(str(d), is_fastq=False, **kw)


def _plain(k):
    return [b">p%d_%d\nACGT\n" % (k, j) * (j + 1) if j in (0, 4) else b"" for j in range(8)]


def test_plain_and_gz_calls_mix_into_one_valid_file(tmp_path):
    rep = _open(tmp_path, zip_out=True)
    a, b, c = _plain(1), [b">g%d\nTTGCA\n" % j * 3 if j in (0, 4) else b"" for j in range(8)], _plain(3)
    try:
        rep.add_fastx(a)
        rep.add_fastx_gz([gzip.compress(x[:9], mtime=0) + gzip.compress(x[9:], mtime=0) if x else b"" for x in b])      # two members per stream
        rep.add_fastx(c)
        rep.add_fastx_gz([gzip.compress(x, mtime=0) if x else b"" for x in b])                                          # and the file ends on raw members
    finally:
        rep.close()
    for j, name in ((0, "aligned.fa.gz"), (4, "other.fa.gz")):
        assert gzip.open(os.path.join(str(tmp_path), name), "rb").read() == a[j] + b[j] + c[j] + b[j], name


def test_gz_members_first_and_a_file_that_gets_nothing(tmp_path):
    rep = _open(tmp_path, zip_out=True)
    try:
        rep.add_fastx_gz([gzip.compress(b">x\nAC\n") if j == 0 else b"" for j in range(8)])
        rep.add_fastx([b">y\nGT\n" if j == 0 else b"" for j in range(8)])
    finally:
        rep.close()
    assert gzip.open(os.path.join(str(tmp_path), "aligned.fa.gz"), "rb").read() == b">x\nAC\n>y\nGT\n"
    assert gzip.open(os.path.join(str(tmp_path), "other.fa.gz"), "rb").read() == b""


def test_denovo_members(tmp_path):
    rep = _open(tmp_path, fastx=False, other=False, denovo=True, zip_out=True)
    try:
        rep.add_denovo([b">a\nAC\n", b"", b"", b""])
        rep.add_denovo_gz([gzip.compress(b">b\nGT\n"), b"", b"", b""])
        off = (C.c_uint64 * 5)
        blob = gzip.compress(b">c\nAA\n")
        assert rep.L.smr_report_add_denovo_gz(rep.h, blob, off(0, 0, len(blob), len(blob), len(blob))) == ERR_ARG      # no such file
        assert rep.L.smr_report_add_denovo_gz(rep.h, blob, off(0, len(blob), len(blob), 5, len(blob))) == ERR_ARG      # offsets decrease
        assert rep.L.smr_report_add_fastx_gz(rep.h, blob, (C.c_uint64 * 9)(0, *([len(blob)] * 8))) == ERR_ARG          # aligned.* is not open
    finally:
        rep.close()
    assert gzip.open(os.path.join(str(tmp_path), "aligned_denovo.fa.gz"), "rb").read() == b">a\nAC\n>b\nGT\n"


def test_refusals_append_nothing(tmp_path):
    blob = gzip.compress(b">c\nAA\n")
    n = len(blob)
    off9 = C.c_uint64 * 9
    rep = _open(tmp_path / "plain", zip_out=False)
    try:
        assert rep.L.smr_report_add_fastx_gz(rep.h, blob, off9(0, *([n] * 8))) == ERR_ARG and b"zip_out" in rep.L.smr_report_last_error(rep.h)
        assert rep.L.smr_report_add_fastx_gz(rep.h, blob, None) == ERR_ARG and rep.L.smr_report_add_fastx_gz(None, blob, off9()) == ERR_ARG
    finally:
        rep.close()
    assert open(os.path.join(str(tmp_path / "plain"), "aligned.fa"), "rb").read() == b""
    rep = _open(tmp_path / "zip", zip_out=True)
    try:
        assert rep.L.smr_report_add_fastx_gz(rep.h, blob, off9(0, 0, n, n, n, n, n, n, n)) == ERR_ARG              # aligned[1] has no open file
        assert b"no open file" in rep.L.smr_report_last_error(rep.h)
        assert rep.L.smr_report_add_fastx_gz(rep.h, blob, off9(0, n, n, n, n, n, n, n, n - 1)) == ERR_ARG          # offsets decrease: aligned[0] is not written either
        assert rep.L.smr_report_add_fastx_gz(rep.h, None, off9(0, n, n, n, n, n, n, n, n)) == ERR_ARG              # bytes without a buffer
        assert rep.L.smr_report_add_fastx_gz(rep.h, None, off9()) == 0                                               # eight empty streams
    finally:
        rep.close()
    assert gzip.open(os.path.join(str(tmp_path / "zip"), "aligned.fa.gz"), "rb").read() == b""


def test_a_report_without_gz_calls_writes_what_it_always_wrote(tmp_path):
    """one gzip member per file, made by zlib at its default level from all the bytes in call order: the same calls give the bytes of
    zlib's own gzopen / gzwrite / gzclose (Python's gzip.GzipFile writes a name and an mtime, so the comparison is against zlib.compressobj
    with a gzip wrapper, whose header is the one gzopen writes but for the OS byte)"""
    import zlib
    rep = _open(tmp_path, zip_out=True)
    a, c = _plain(1), _plain(3)
    try:
        rep.add_fastx(a)
        rep.add_fastx(c)
    finally:
        rep.close()
    for j, name in ((0, "aligned.fa.gz"), (4, "other.fa.gz")):
        got = open(os.path.join(str(tmp_path), name), "rb").read()
        z = zlib.compressobj(zlib.Z_DEFAULT_COMPRESSION, zlib.DEFLATED, 31)
        want = z.compress(a[j] + c[j]) + z.flush()
        assert got[:3] == b"\x1f\x8b\x08" and got[3] == 0, "a header with flags (a name)"
        assert got[10:] == want[10:] and len(got) == len(want), name                                # the same DEFLATE data, CRC-32 and ISIZE: one member
        assert gzip.decompress(got) == a[j] + c[j]
