"""CPU: the report side of gzipping the SAM and BLAST reports on the device -- smr_report_add_rows_gz / smr_report_add_pairwise_gz keep gzip
members made elsewhere with the rows of their (index, part), and smr_report_close writes every key's pieces in call order: plain rows through
zlib, members as they are.  The members here are Python's gzip.compress; the files are read back with Python's gzip and zlib, which inflate a
multi-member file the way any downstream tool has to.  The yardstick of every mixed report is the report that got the same rows through the
plain calls alone."""
import ctypes as C
import gzip
import os
import zlib

from helpers import rows
from helpers.rowsgzdev import members
from sortmerna_amd import report
from test_gpu_pairwise import HDR, SEQ, _one_record
from test_gpu_rows import syn_part

ERR_ARG = -1
KEYS = [(0, 0), (0, 1)]


def _open(d, zip_out, sam=True, cols=(), pairwise=False, sq=True):
    os.makedirs(str(d), exist_ok=True)
    ix, _ = syn_part()
    rep = report.Report(str(d), is_fastq=False, fastx=False, other=False, sam=sam, blast_cols=None if cols is None else list(cols), blast_pairwise=pairwise,
                        sam_sq=sq, cmdline="the command line", zip_out=zip_out)
    for k, (lam, K, fr, fq) in rows.DB.items():
        rep.set_db(k, lam, K, fr, fq)
    for key in KEYS:
        rep.set_part(key[0], key[1], ix)
    return rep


def _read(d, name):
    return gzip.open(os.path.join(str(d), name + ".gz"), "rb").read()


def _gz(text, pieces=1):
    """`text` as gzip members"""
    step = (len(text) + pieces - 1) // pieces
    return b"".join(gzip.compress(text[at:at + step], mtime=0) for at in range(0, len(text), step))


def _rows_of(key, tag, n):
    return (b"".join(b"%s%d\t0\tref%d_%d\t1\t255\t4M\t*\t0\t0\tACGT\t*\tAS:i:8\tNM:i:0\n" % (tag, i, key[0], key[1]) for i in range(n)),
            b"".join(b"%s%d\tref%d_%d\t100\t4\t0\t0\t1\t4\t1\t4\t0.1\t8\n" % (tag, i, key[0], key[1]) for i in range(n)))


# the calls of one report: (key, tag, how): "plain" | "gz" | "add" (the host writer, one read)
CALLS = [((0, 1), b"a", "gz"), ((0, 1), b"b", "plain"), ((0, 0), b"c", "plain"), ((0, 0), b"d", "add"), ((0, 0), b"e", "gz"), ((0, 1), b"f", "gz"), ((0, 0), b"g", "plain")]


def _feed(rep, mixed):
    rec = _one_record(None)
    for j, (key, tag, how) in enumerate(CALLS):
        sam, blast = _rows_of(key, tag, 40 + j)
        if how == "add":
            rep.add(HDR, SEQ, None, rec)
        elif how == "gz" and mixed:
            rep.add_rows_gz(key[0], key[1], _gz(sam, 2), _gz(blast, 1 + j % 2))
        else:
            rep.add_rows(key[0], key[1], sam, blast)


def test_rows_gz_and_plain_calls_mix_into_the_file_of_the_plain_calls(tmp_path):
    for tag, mixed, zip_out in (("plain", False, False), ("zip", False, True), ("mixed", True, True)):
        rep = _open(tmp_path / tag, zip_out)
        try:
            _feed(rep, mixed)
        finally:
            rep.close()
    for name in ("aligned.sam", "aligned.blast"):
        want = open(os.path.join(str(tmp_path / "plain"), name), "rb").read()
        assert want.count(b"\n") > 250
        assert _read(tmp_path / "zip", name) == want, name
        assert _read(tmp_path / "mixed", name) == want, name
        got = members(open(os.path.join(str(tmp_path / "mixed"), name + ".gz"), "rb").read())
        assert len(got) > 6 and b"".join(got) == want, (name, len(got))             # zlib walks the file member by member
    sam = _read(tmp_path / "mixed", "aligned.sam").split(b"\n")
    ix, _ = syn_part()
    n_sq = sum(1 for l in sam if l.startswith(b"@SQ\t"))
    assert sam[0].startswith(b"@HD\t") and n_sq > 1 and all(l.startswith(b"@SQ\t") for l in sam[1:1 + n_sq]) and sam[1 + n_sq] == b"@PG\tID:sortmerna\tVN:1.0\tCL:the command line"
    # keys in key order, the pieces of a key in call order
    tags = [l[:1] for l in sam[2 + n_sq:] if l]
    order = [t for k, t, _ in sorted(CALLS, key=lambda c: c[0]) if t != b"d"]
    assert [t for i, t in enumerate(tags) if t != b"r" and (i == 0 or tags[i - 1] != t)] == order, tags
    assert tags.count(b"r") == 1 and tags.index(b"r") == tags.index(b"e") - 1                    # the host writer's row, between "c" and "e"


def test_pairwise_gz_and_plain_calls_mix(tmp_path):
    texts = {(0, 1): [b"Sequence ID: x\nQuery ID: q%d\n\n" % i * 30 for i in range(3)], (0, 0): [b"Sequence ID: y\nQuery ID: p%d\n\n" % i * 50 for i in range(2)]}
    for tag, mixed, zip_out in (("plain", False, False), ("mixed", True, True)):
        rep = _open(tmp_path / tag, zip_out, sam=False, cols=None, pairwise=True)
        try:
            for key in ((0, 1), (0, 0)):
                for j, t in enumerate(texts[key]):
                    if mixed and j != 1:
                        rep.add_pairwise_gz(key[0], key[1], _gz(t, 2))
                    else:
                        rep.add_pairwise(key[0], key[1], t)
            if mixed:
                assert rep.L.smr_report_add_pairwise_gz(rep.h, 0, 0, None, 0) == 0                   # an empty stream is nothing
        finally:
            rep.close()
    want = open(os.path.join(str(tmp_path / "plain"), "aligned.blast"), "rb").read()
    assert want == b"".join(texts[(0, 0)]) + b"".join(texts[(0, 1)])
    assert _read(tmp_path / "mixed", "aligned.blast") == want


def test_refusals_append_nothing(tmp_path):
    sam, blast = _rows_of((0, 0), b"x", 5)
    gs, gb = _gz(sam), _gz(blast)
    off = C.c_uint64 * 3
    both = off(0, len(gs), len(gs) + len(gb))

    def err(rep):
        return rep.L.smr_report_last_error(rep.h).decode()

    rep = _open(tmp_path / "not_zip", False, cols=())
    try:
        assert rep.L.smr_report_add_rows_gz(rep.h, 0, 0, gs + gb, both) == ERR_ARG and "smr_report_add_rows_gz" in err(rep) and "zip_out" in err(rep)
        assert rep.L.smr_report_add_pairwise_gz(rep.h, 0, 0, gs, len(gs)) == ERR_ARG and "smr_report_add_pairwise_gz" in err(rep) and "zip_out" in err(rep)
    finally:
        rep.close()
    assert rows.strip_header(open(os.path.join(str(tmp_path / "not_zip"), "aligned.sam"), "rb").read()) == b""
    assert open(os.path.join(str(tmp_path / "not_zip"), "aligned.blast"), "rb").read() == b""
    rep = _open(tmp_path / "sam_only", True, cols=None)
    try:
        assert rep.L.smr_report_add_rows_gz(rep.h, 0, 0, gs + gb, both) == ERR_ARG and "blast_tabular" in err(rep)        # BLAST rows, no BLAST report: the SAM rows are not kept either
        assert rep.L.smr_report_add_rows_gz(rep.h, 0, 0, gs + gb, off(0, len(gs), len(gs) - 1)) == ERR_ARG and "decrease" in err(rep)
        assert rep.L.smr_report_add_rows_gz(rep.h, 0, 0, gs + gb, off(1, 0, 0)) == ERR_ARG
        assert rep.L.smr_report_add_rows_gz(rep.h, 0, 7, gs, off(0, len(gs), len(gs))) == ERR_ARG and "registered" in err(rep)
        assert rep.L.smr_report_add_rows_gz(rep.h, 0, 0, None, off(0, len(gs), len(gs))) == ERR_ARG                       # rows without bytes
        assert rep.L.smr_report_add_rows_gz(rep.h, 0, 0, gs, None) == ERR_ARG and rep.L.smr_report_add_rows_gz(None, 0, 0, gs, both) == ERR_ARG
        assert rep.L.smr_report_add_pairwise_gz(rep.h, 0, 0, gs, len(gs)) == ERR_ARG and "blast_pairwise" in err(rep)
        assert rep.L.smr_report_add_rows_gz(rep.h, 0, 0, None, off(0, 0, 0)) == 0                                         # two empty streams
    finally:
        rep.close()
    assert rows.strip_header(_read(tmp_path / "sam_only", "aligned.sam")) == b""
    assert not os.path.exists(os.path.join(str(tmp_path / "sam_only"), "aligned.blast.gz"))
    rep = _open(tmp_path / "blast_only", True, sam=False, cols=())
    try:
        assert rep.L.smr_report_add_rows_gz(rep.h, 0, 0, gs + gb, both) == ERR_ARG and "sam" in err(rep)                  # SAM rows, no SAM report: the BLAST rows are not kept either
    finally:
        rep.close()
    assert _read(tmp_path / "blast_only", "aligned.blast") == b""
    rep = _open(tmp_path / "pair_and_tab", True, sam=False, cols=(), pairwise=True)
    try:
        assert rep.L.smr_report_add_pairwise_gz(rep.h, 0, 0, gs, len(gs)) == ERR_ARG and "blast_tabular" in err(rep)
    finally:
        rep.close()
    rep = _open(tmp_path / "pair", True, sam=False, cols=None, pairwise=True)
    try:
        assert rep.L.smr_report_add_pairwise_gz(rep.h, 0, 7, gs, len(gs)) == ERR_ARG and "registered" in err(rep)
        assert rep.L.smr_report_add_pairwise_gz(rep.h, 0, 0, None, len(gs)) == ERR_ARG
    finally:
        rep.close()
    assert _read(tmp_path / "pair_and_tab", "aligned.blast") == b"" and _read(tmp_path / "pair", "aligned.blast") == b""


def test_a_report_without_gz_calls_writes_what_it_always_wrote(tmp_path):
    """one gzip member per file, made by zlib at its default level from all the bytes in key order: the bytes of zlib's own gzopen / gzwrite /
    gzclose, as test_gzip_report_cpu.py compares them (against zlib.compressobj with a gzip wrapper, whose header is gzopen's but for the OS byte)"""
    for tag, zip_out in (("plain", False), ("zip", True)):
        rep = _open(tmp_path / tag, zip_out)
        try:
            _feed(rep, False)
        finally:
            rep.close()
    for name in ("aligned.sam", "aligned.blast"):
        text = open(os.path.join(str(tmp_path / "plain"), name), "rb").read()
        got = open(os.path.join(str(tmp_path / "zip"), name + ".gz"), "rb").read()
        z = zlib.compressobj(zlib.Z_DEFAULT_COMPRESSION, zlib.DEFLATED, 31)
        want = z.compress(text) + z.flush()
        assert got[:3] == b"\x1f\x8b\x08" and got[3] == 0, "a header with flags (a name)"
        assert got[10:] == want[10:] and len(got) == len(want), name                                 # the same DEFLATE data, CRC-32 and ISIZE: one member
        assert len(members(got)) == 1 and gzip.decompress(got) == text
