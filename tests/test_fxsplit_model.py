"""CPU, no kernels: the host model of smr_fastx_split (helpers/fxsplit.py) against the report writer that is character-exact against the
reference (smr_report_add / smr_report_add_pair, test_reports_cpu.py): every valid combination of paired_in / paired_out / out2 / sout, each
of the four hit patterns of a pair, FASTA and FASTQ.  The files the writer makes must equal the model's streams; a file that is not there
matches an empty stream.  Then the two report calls that take the streams: smr_report_add_fastx must write the same files, smr_report_skip_fastx
must keep smr_report_add / _add_pair off them and nothing else."""
import gzip
import os
import struct

import pytest

import sortmerna_amd as smr
from sortmerna_amd.report import Report
from helpers.fxsplit import VALID_OPTS, expected_streams, num_out, opts_id, pair_files

HIT_RECORD = struct.pack("<6I3BHiIQIIQ", 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 16, 0, 0, 0)      # Read::toBinString of a hit without stored alignments
PAIR_HITS = [(0, 0), (1, 0), (0, 1), (1, 1), (1, 1), (0, 1), (1, 0), (0, 0)]


def text_of(fastq):
    out = []
    for i in range(16):
        seq = b"ACGTNacgtn"[: 1 + i % 10] * (1 + i % 3)
        if fastq:
            out.append(b"@r%d %s\n%s \t\n+r%d\n%s\n" % (i, b"x" * i, seq, i, b"I" * len(seq)))
        else:
            out.append(b">r%d %s\r\n%s\n%s\n" % (i, b"x" * i, seq[:3], seq[3:]))
    return b"".join(out)


def suffixes(o):
    n = num_out(o)
    if n == 4:
        return ["_paired_fwd", "_paired_rev", "_singleton_fwd", "_singleton_rev"]
    if n == 2:
        return ["_fwd", "_rev"] if o.get("out2") else ["_paired", "_singleton"]
    return [""]


def files_as_streams(out_dir, o, fastq, zipped=False):
    ext = ".fq" if fastq else ".fa"
    sfx = suffixes(o) + [None] * 4
    out = []
    for base in ("aligned", "other"):
        for j in range(4):
            path = os.path.join(out_dir, base + sfx[j] + ext + (".gz" if zipped else "")) if sfx[j] is not None else None
            if path is None or not os.path.exists(path):
                out.append(b"")
            else:
                out.append(gzip.open(path, "rb").read() if zipped else open(path, "rb").read())
    return out


@pytest.fixture(scope="module", params=[True, False], ids=["fastq", "fasta"])
def reads(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("model") / "reads.txt")
    with open(path, "wb") as f:
        f.write(text_of(request.param))
    r = smr.Reads.from_fastx_text(path)
    yield r
    r.free()


def mate(reads, i, hit):
    h, s, q = reads.record_text(i)
    return (h, s, q if reads.is_fastq else None, HIT_RECORD if hit else b"")


def write_pairs(rep, reads, hits):
    for k in range(reads.count // 2):
        rep.add_pair(mate(reads, 2 * k, hits[2 * k]), mate(reads, 2 * k + 1, hits[2 * k + 1]))


def test_a_record_goes_to_one_file_only():
    for o in VALID_OPTS:
        for hit in [(0, 0), (1, 0), (0, 1), (1, 1)]:
            al, ot = pair_files(o, hit)
            for i in range(2):
                assert (al[i] is None) != (ot[i] is None), (o, hit, i)


@pytest.mark.parametrize("o", VALID_OPTS, ids=opts_id)
def test_the_model_is_the_writer_for_pairs(o, reads, tmp_path):
    hits = [h for p in PAIR_HITS for h in p]
    rep = Report(str(tmp_path), reads.is_fastq, fastx=True, other=True, **o)
    write_pairs(rep, reads, hits)
    rep.close()
    assert files_as_streams(str(tmp_path), o, reads.is_fastq) == expected_streams(reads, hits, dict(layout=1, **o))
    for al, ot in [(True, False), (False, True)]:
        d = tmp_path / ("a%d" % al)
        os.makedirs(d)
        rep = Report(str(d), reads.is_fastq, fastx=al, other=ot, **o)
        write_pairs(rep, reads, hits)
        rep.close()
        assert files_as_streams(str(d), o, reads.is_fastq) == expected_streams(reads, hits, dict(layout=1, aligned=al, other=ot, **o))


def test_the_model_is_the_writer_for_single_reads(reads, tmp_path):
    hits = [h for p in PAIR_HITS for h in p]
    rep = Report(str(tmp_path), reads.is_fastq, fastx=True, other=True)
    for i in range(reads.count):
        rep.add(*mate(reads, i, hits[i]))
    rep.close()
    assert files_as_streams(str(tmp_path), {}, reads.is_fastq) == expected_streams(reads, hits, dict(layout=0))


@pytest.mark.parametrize("zipped", [False, True], ids=["plain", "gzip"])
@pytest.mark.parametrize("o", [VALID_OPTS[0], VALID_OPTS[7]], ids=opts_id)
def test_add_fastx_writes_the_streams_and_skip_fastx_keeps_the_writer_off_them(o, zipped, reads, tmp_path):
    hits = [h for p in PAIR_HITS for h in p]
    streams = expected_streams(reads, hits, dict(layout=1, **o))
    rep = Report(str(tmp_path), reads.is_fastq, fastx=True, other=True, blast_cols=[], zip_out=zipped, **o)
    rep.skip_fastx(True)
    write_pairs(rep, reads, hits)                                   # (would write every record a second time)
    rep.add_fastx(streams[:4] + [b""] * 4)                          # in two calls: the streams are appended
    rep.add_fastx([b""] * 4 + streams[4:])
    rep.close()
    assert files_as_streams(str(tmp_path), o, reads.is_fastq, zipped) == streams
    assert os.path.exists(os.path.join(str(tmp_path), "aligned.blast" + (".gz" if zipped else "")))


def test_add_fastx_refuses_a_stream_without_a_file(reads, tmp_path):
    hits = [h for p in PAIR_HITS for h in p]
    streams = expected_streams(reads, hits, dict(layout=0))
    rep = Report(str(tmp_path), reads.is_fastq, fastx=False, other=True)
    with pytest.raises(smr.SmrError) as x:
        rep.add_fastx(streams)                                      # aligned[0] is not empty, aligned.* is not open
    assert "rc=-1" in str(x.value)
    with pytest.raises(smr.SmrError):
        rep.add_fastx([b""] * 5 + [b"x"] + [b""] * 2)               # other[1] does not exist under these options
    rep.add_fastx([b""] * 4 + streams[4:])
    rep.close()
    assert files_as_streams(str(tmp_path), {}, reads.is_fastq) == [b""] * 4 + streams[4:]
