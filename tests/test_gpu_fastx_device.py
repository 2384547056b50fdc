"""smr_reads_upload_fastx*: FASTA/FASTQ text parsed and 2-bit packed by kernels (csrc/smr_fastx.hpp), straight into the resident batch.

The yardstick of every test is the host parser on the same bytes (the bytes written to a file, Reads.from_fastx_text); it is never the code under
test.  Every comparison is for equality.
1. packing at its boundaries: read lengths around the 16- and 32-letter words, sequences starting at every byte phase, every kind of letter,
   quality lines that start with '@' and '+', trailing blanks, wrapped FASTA; LF, CRLF, no final newline, blank lines around;
2. scan boundaries: record counts around a wave, a block of lines, and one more than the lines a block of the line kernel can find; a header
   longer than a block's tile of text; a wrapped record whose lines cross a tile edge;
3. irregular and malformed text: the host's Reads or the host's message;
4. the batch is the uploaded one: golden cases aligned after upload_fastx (file, batch=1, .gz) against upload_reads and the stored records;
5. guards.
In 1, 2 and 4 every case must report the device path.  test_emu_fastx_device.py runs the same bodies on the emulator."""
import ctypes as C
import gzip
import os
import random

import pytest

import sortmerna_amd as smr
from helpers import golden
from helpers.cases import build_case

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_IO, ERR_CAPACITY, ERR_STATE = -1, -2, -4, -5
FX_TILE = 4096                # csrc/smr_fastx.hpp: text bytes per block of k_fx_count / k_fx_lines = the most lines one block can find
FX_LBLOCK = 1024              # ... lines / records per block of the record kernels
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, 150, 5000]
ALPHABET = [bytes([c]) for c in b"ACGTUacgtuNnRYKM-. "] + ["é".encode()]          # (two bytes >= 0x80)
DRESSINGS = ["lf", "crlf", "no_final_newline", "blank_lines_around"]
SCAN_COUNTS = [1, 63, 64, 65, 255, 256, 257, FX_TILE + 1]


def letters(rng, n, mark=None):
    """n bytes of sequence text, whole letters only; mark: a byte to put at offset 5"""
    out, size = [], 0
    while size < n:
        t = mark if (mark and size == 5) else rng.choice(ALPHABET if n - size > 1 else ALPHABET[:-1])
        out.append(t)
        size += len(t)
    return b"".join(out)


def dress(text, how):
    if how == "crlf":
        return text.replace(b"\n", b"\r\n")
    if how == "no_final_newline":
        return text[:-1] if text.endswith(b"\n") else text
    if how == "blank_lines_around":
        return b"\n\n\n" + text + b"\n\n"
    return text


def boundary_text(fastq):
    rng = random.Random(20261018)
    lens = LENGTHS + [150, 33]                                  # 17 records: header lines of 1 .. 17 bytes
    widths = [1, 7, 16, 60, 61]
    out = []
    for i, n in enumerate(lens):
        hdr = (b"@" if fastq else b">") + (b"r%016d" % i)[:i]
        seq = letters(rng, n, (b"@" if i % 4 == 0 else b">") if n >= 48 and i % 2 == 0 else None)      # a record-start letter inside a sequence line
        tail = b" \t\r" if i in (4, 9) else b""
        if fastq:
            qual = (b"@" if i % 2 else b"+") + b"I" * (n - 1) if n else b""
            out += [hdr, seq + tail, b"+" + (hdr[1:] if i % 3 == 0 else b""), qual]
        else:
            w = 60 if n == 5000 else widths[(i + 3) % 5]
            lines = [seq[k:k + w] for k in range(0, n, w)]
            if lines:
                lines[-1] += tail
            if i == 11:
                lines.insert(1, b"")                            # an empty line inside a record
            out += [hdr] + lines
    if not fastq:
        out.append(b">last_has_no_sequence_line")
    return b"\n".join(out) + b"\n"


def scan_text(fastq, n_rec):
    rng = random.Random(n_rec)
    out = []
    for i in range(n_rec):
        seq = letters(rng, 1 + (i * 7) % 40)
        if fastq:
            out += [b"@%d" % i, seq, b"+", b"I" * len(seq)]
        else:
            out += [b">%d" % i, seq]
    return b"\n".join(out) + b"\n"


def long_text(fastq):
    """a header longer than a block's tile of text; a 5 000-letter record wrapped at 60, whose lines cross a tile edge"""
    rng = random.Random(7)
    seq = letters(rng, 5000)
    if fastq:
        return b"@a\nACGT\n+\nIIII\n@" + b"h" * (FX_TILE + 100) + b"\n" + seq + b"\n+\n" + b"I" * 5000 + b"\n@z\nNACGT\n+\nIIIII\n"
    wrapped = b"\n".join(seq[k:k + 60] for k in range(0, 5000, 60))
    return b">a\nACGT\n>" + b"h" * (FX_TILE + 100) + b"\nACGTN\n>long\n" + wrapped + b"\n>z\nAC\n"


def is_regular(data):
    """the definition of INTEGRATION.md ("Parsing and packing on the device"), restated by walking the lines"""
    first = 0
    while first < len(data) and data[first:first + 1] in (b"\n", b"\r"):
        first += 1
    if first >= len(data):
        return False
    if data[first:first + 1] == b">":
        return True
    if data[first:first + 1] != b"@":
        return False
    body = data[first:]
    lines = body[:-1].split(b"\n") if body.endswith(b"\n") else body.split(b"\n")
    blank = [ln in (b"", b"\r") for ln in lines]
    last = max(i for i, b in enumerate(blank) if not b) + 1
    n_rec = (last + 3) // 4
    return 4 * n_rec <= len(lines) and all(lines[4 * k][:1] == b"@" for k in range(n_rec)) and all(blank[4 * n_rec:])


def same_reads(got, want, what, view=False):
    assert (got.count, got.total_len, got.min_len, got.max_len, got.is_fastq) == (want.count, want.total_len, want.min_len, want.max_len, want.is_fastq), what
    for i in range(want.count):
        assert got.record_text(i) == want.record_text(i), "%s: record %d" % (what, i)
    if view:
        assert got.digest == 0, what
        with pytest.raises(smr.SmrError):
            got.slice(0, 0)
    else:
        assert got.digest == want.digest, what


def on_device_equals_host(e, data, tmp_path, what):
    assert is_regular(data), what
    path = os.path.join(str(tmp_path), "reads.txt")
    with open(path, "wb") as f:
        f.write(data)
    want = smr.Reads.from_fastx_text(path)
    try:
        for view in (False, True):
            for src in (data, path):
                got = e.upload_fastx(src, 2, view=view)
                try:
                    info = e.fastx_info()
                    assert info[0] == 0, "%s: the host parser ran" % what
                    assert info[2] == want.count and info[3] == len(data), what
                    same_reads(got, want, what, view)
                finally:
                    got.free()
    finally:
        want.free()


# ------------------------------------------------------------------------------------------------ 1. packing at its boundaries
def boundaries_body(fastq, how, tmp_path):
    e = smr.Engine(0)
    try:
        on_device_equals_host(e, dress(boundary_text(fastq), how), tmp_path, "%s, %s" % ("fastq" if fastq else "fasta", how))
    finally:
        e.close()


@pytest.mark.parametrize("how", DRESSINGS)
@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_packing_at_its_boundaries(fastq, how, tmp_path):
    boundaries_body(fastq, how, tmp_path)


# ------------------------------------------------------------------------------------------------ 2. scan boundaries
def scan_body(fastq, n_rec, tmp_path):
    e = smr.Engine(0)
    try:
        on_device_equals_host(e, scan_text(fastq, n_rec), tmp_path, "%d records" % n_rec)
    finally:
        e.close()


def long_body(fastq, tmp_path):
    e = smr.Engine(0)
    try:
        on_device_equals_host(e, long_text(fastq), tmp_path, "long header, long record")
    finally:
        e.close()


@pytest.mark.parametrize("n_rec", SCAN_COUNTS)
@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_scan_boundaries(fastq, n_rec, tmp_path):
    scan_body(fastq, n_rec, tmp_path)


@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_a_header_and_a_record_longer_than_a_tile(fastq, tmp_path):
    long_body(fastq, tmp_path)


# ------------------------------------------------------------------------------------------------ golden runs (3, 4, 5)
def slots_of(p):
    return p.num_alignments if p.num_alignments > 0 else 32


def case_run(e, case, tmp_path, upload):
    """golden case `case` aligned on e after upload(reads path, slots) put the reads in place -> (records, counters, is_hit)"""
    g = golden.load()[case]
    idx, seqs = build_case(case, tmp_path)
    params = {k: v for k, v in g["params"].items() if k not in ("max_mb", "evalue", "lnwin")}
    plist = [smr.default_params(minimal_score=d["minimal_score"], **params) for d in idx]
    try:
        upload(golden.inputs(case)[1], slots_of(plist[0]))
        smr.align(e, None, [d["parts"] for d in idx], plist)
        assert e.n_reads == len(seqs)
        return e.records(), e.counters(len(idx)), [e.is_hit(i) for i in range(len(seqs))]
    finally:
        for d in idx:
            for ix in d["parts"]:
                ix.free()


def host_upload(e):
    def up(path, slots):
        r = smr.Reads.from_fastx_text(path)
        e.upload_reads(r, slots)
        r.free()
    return up


def device_upload(e, how, tmp_path):
    def up(path, slots):
        data = open(path, "rb").read()
        if how == "file":
            r = e.upload_fastx(path, slots)
        elif how == "gz":
            gz = os.path.join(str(tmp_path), "reads.fasta.gz")
            with gzip.open(gz, "wb") as f:
                f.write(data)
            r = e.upload_fastx(gz, slots)
        else:                                                   # into batch 1 while batch 0 is selected
            e.select_batch(0)
            r = e.upload_fastx(data, slots, batch=1)
            e.select_batch(1)
        assert e.fastx_info()[0] == 0 and e.fastx_info()[3] == len(data), "the host parser ran"
        r.free()
    return up


# ------------------------------------------------------------------------------------------------ 3. irregular and malformed text
REC = b"@a\nACGTN\n+\nIIIII\n"
IRREGULAR = {
    "blank line between records": REC + b"\n" + REC,
    "cut after 1 line": REC + b"@b\n",
    "cut after 2 lines": REC + b"@b\nACGT\n",
    "cut after 3 lines": REC + b"@b\nACGT\n+\n",
    "cr in front of a record": REC + b"\r@b\nAC\n+\nII\n",
    "stray letter between records": REC + b"x\n" + REC,
    "stray letter behind blank lines": REC + b"\n\nA\n",
    "starts with A": b"ACGT\n" + REC,
    "empty": b"",
    "blank bytes only": b"\n\r\n\r\n",
    "fasta, then nothing": b">only\n",
}


def irregular_body(tmp_path):
    e = smr.Engine(0)
    try:
        for what, data in IRREGULAR.items():
            path = os.path.join(str(tmp_path), "irregular.txt")
            with open(path, "wb") as f:
                f.write(data)
            try:
                want, why = smr.Reads.from_fastx_text(path), None
            except smr.SmrError as x:
                want, why = None, str(x).split(": ", 1)[1]      # "<path>: <what is wrong> (rc=..)"
            for src in (path, data):
                if want is None:
                    with pytest.raises(smr.SmrError) as x:
                        e.upload_fastx(src)
                    said = str(x.value).split(": ", 1)[1]
                    assert said == (why if src is path else why.split(": ", 1)[1]), what
                else:
                    got = e.upload_fastx(src)
                    same_reads(got, want, what)
                    assert e.fastx_info()[2] == want.count
                    got.free()
            if want is not None:
                want.free()
        # the context is still good for a run
        recs, _, _ = case_run(e, "t9", tmp_path, device_upload(e, "file", tmp_path))
        assert recs == golden.records("t9")
    finally:
        e.close()


def test_irregular_and_malformed_text(tmp_path):
    irregular_body(tmp_path)


# ------------------------------------------------------------------------------------------------ 4. the batch is the uploaded one
GOLDEN_CASES = [("real_default", "file"), ("t9", "file"), ("t9", "batch"), ("t9", "gz")]


def golden_body(case, how, tmp_path):
    e = smr.Engine(0)
    try:
        want = case_run(e, case, tmp_path, host_upload(e))
        e.select_batch(0)
        got = case_run(e, case, tmp_path, device_upload(e, how, tmp_path))
        assert got[0] == want[0] == golden.records(case)
        assert got[1] == want[1] and got[2] == want[2]
    finally:
        e.close()


@pytest.mark.parametrize("case,how", GOLDEN_CASES)
def test_the_batch_is_the_uploaded_one(case, how, tmp_path):
    golden_body(case, how, tmp_path)


# ------------------------------------------------------------------------------------------------ 5. guards
def guards_body(tmp_path):
    e = smr.Engine(0)
    L = e.L
    try:
        before = case_run(e, "t9", tmp_path, device_upload(e, "file", tmp_path))[0]
        text = C.create_string_buffer(REC)
        h = C.c_void_p()
        err = C.create_string_buffer(256)
        missing = os.path.join(str(tmp_path), "no_such_file.fq").encode()
        refusals = [
            (lambda: L.smr_reads_upload_fastx(e.h, None, 0, 1, 0, C.byref(h)), ERR_ARG),
            (lambda: L.smr_reads_upload_fastx(None, text, len(REC), 1, 0, C.byref(h)), ERR_ARG),
            (lambda: L.smr_reads_upload_fastx_batch(e.h, 1, None, 0, 1, 0, None), ERR_ARG),
            (lambda: L.smr_reads_upload_fastx_batch(e.h, 16, text, len(REC), 1, 0, None), ERR_ARG),
            (lambda: L.smr_reads_upload_fastx_batch(e.h, 0, text, len(REC), 1, 0, C.byref(h)), ERR_STATE),          # batch 0 is the selected one
            (lambda: L.smr_reads_upload_fastx_file(e.h, None, 1, 0, C.byref(h), err, 256), ERR_ARG),
            (lambda: L.smr_reads_upload_fastx_file(e.h, missing, 1, 0, C.byref(h), err, 256), ERR_IO),
            (lambda: L.smr_reads_upload_fastx(e.h, text, 2 ** 32 - 64, 1, 0, C.byref(h)), ERR_CAPACITY),             # decided before the text is touched
            (lambda: L.smr_reads_upload_fastx(e.h, C.create_string_buffer(b"ACGT\n"), 5, 1, 0, C.byref(h)), ERR_IO),
            (lambda: L.smr_fastx_info(e.h, None), ERR_ARG),
        ]
        for k, (call, rc) in enumerate(refusals):
            assert call() == rc, "refusal %d" % k
            e.fetch()
            assert e.records() == before, "refusal %d changed the batch" % k
        assert b"no_such_file" in err.value
        # a view is not a batch to upload or slice
        v = e.upload_fastx(REC, view=True)
        assert L.smr_reads_upload(e.h, v.h, 1) == ERR_STATE and L.smr_reads_upload_batch(e.h, 1, v.h, 1) == ERR_STATE
        assert L.smr_reads_slice(v.h, 0, 1, C.byref(h)) == ERR_STATE
        assert (v.count, v.total_len, v.record_text(0)) == (1, 5, ("@a", "ACGTN", "IIIII"))
        v.free()
    finally:
        e.close()


def test_guards(tmp_path):
    guards_body(tmp_path)
