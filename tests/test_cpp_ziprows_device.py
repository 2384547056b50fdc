"""The C++ host driver (examples/smr_align.cpp) with --ziprows device: under gzipped reports the SAM / BLAST rows come from smr_rows_part_gz +
smr_report_add_rows_gz and the pairwise text from smr_pairwise_part_gz + smr_report_add_pairwise_gz -- gzip members made by the DEFLATE kernels,
cut at line ends, and written as they are when the report closes.  The run must write the files of the --ziprows host run, each equal after
inflation (Python's gzip is the yardstick, and reads the multi-member files the way any downstream tool has to)."""
import os
import subprocess

import pytest

from helpers import golden
from helpers.rowsgzdev import members
from test_cpp_driver import _emu_driver, build_driver
from test_cpp_rows_device import BLAST, _two_db_args
from test_cpp_split_device import _content, _fasta_args, _files, _interleaved_args

BASE = ["--pack", "device", "-zip-out", "1"]


def _same_outputs(exe, args, tmp_path, tag, reports, device):
    """the run with --ziprows host against the run with --ziprows device, both with the `device` switches"""
    outs = {}
    for zr in ("host", "device"):
        outs[zr] = tmp_path / (tag + "_" + zr)
        os.makedirs(outs[zr])
        subprocess.check_call([exe] + args + list(reports) + BASE + list(device) + ["--ziprows", zr, "--out", str(outs[zr])])
    fa = _files(outs["host"])
    assert fa == _files(outs["device"]), tag
    differ = [f for f in fa if _content(str(outs["host"] / f)) != _content(str(outs["device"] / f))]
    assert not differ, (tag, differ)
    for f, flag, least in (("aligned.sam.gz", "--sam", b"\n"), ("aligned.blast.gz", "--blast", b"\n")):
        if flag in reports:
            assert f in fa and os.path.getsize(str(outs["device"] / f)) > 0, (tag, f)
            assert _content(str(outs["device"] / f)).count(least) > 3, "%s: %s holds no rows: the comparison shows nothing" % (tag, f)
            # the members the device made lie behind what zlib made of the header (or are the whole file): the host path writes one member
            n_host, n_dev = (len(members(open(str(outs[zr] / f), "rb").read())) for zr in ("host", "device"))
            assert n_host == 1 and n_dev >= (2 if f == "aligned.sam.gz" else 1), (tag, f, n_host, n_dev)
    return outs


def _case(exe, tmp_path, tag):
    one = _fasta_args("syn_default")
    rows = ["--rows", "device"]
    if tag == "sam":
        _same_outputs(exe, one, tmp_path, tag, ["--sam"], rows)
    elif tag == "sq_blast":                                # BLAST tabular with the optional columns, SAM with its @SQ lines in front
        _same_outputs(exe, one, tmp_path, tag, ["--sam", "-SQ"] + BLAST, rows)
    elif tag == "pairwise":
        _same_outputs(exe, one, tmp_path, tag, ["--blast", "0"], ["--pairwise", "device"])
    elif tag == "two_db":                                  # several (index, part): the members of every key, in key order
        _same_outputs(exe, _two_db_args(), tmp_path, tag, ["--sam"] + BLAST, rows)
    elif tag == "interleaved":
        _same_outputs(exe, _interleaved_args(tmp_path) + ["-paired_out"], tmp_path, tag, ["--sam", "--fastx", "--other"] + BLAST, rows)
    else:                                                  # with --split device --zip device: every report file of the run is made of device members
        _same_outputs(exe, one, tmp_path, tag, ["--sam", "--fastx", "--other"] + BLAST, rows + ["--split", "device", "--zip", "device"])


CASES = ["sam", "sq_blast", "pairwise", "two_db", "interleaved", "split_zip"]


def _refusals(exe, tmp_path):
    one = _fasta_args("syn_default")
    run = lambda args: subprocess.run([exe] + args + ["--out", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    neither = run(one + ["--pack", "device", "-zip-out", "1", "--sam", "--ziprows", "device"])                       # neither --rows device nor --pairwise device
    plain = run(one + ["--pack", "device", "--rows", "device", "--sam", "--ziprows", "device"])                      # a plain reads file: the reports are not gzipped
    off = run(one + ["--pack", "device", "--pairwise", "device", "--blast", "0", "-zip-out", "0", "--ziprows", "device"])
    word = run(one + ["--ziprows", "sometimes"])
    for p in (neither, plain, off, word):
        assert p.returncode != 0 and b"--ziprows" in p.stderr, p.stderr
    assert b"--rows device" in neither.stderr and b"--pairwise device" in neither.stderr and b"not gzipped" not in neither.stderr
    assert b"not gzipped" in plain.stderr and b"not gzipped" in off.stderr and b"--rows device" not in plain.stderr      # each condition has its own message
    assert b"host or device" in word.stderr
    assert not os.listdir(str(tmp_path))                                  # refused before anything was loaded or written
    assert "--ziprows host|device" in subprocess.check_output([exe, "--help"]).decode()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", CASES)
def test_ziprows_device_inflates_to_the_files_of_ziprows_host(tag, tmp_path):
    _case(build_driver(), tmp_path, tag)


@pytest.mark.gpu
def test_ziprows_device_refusals(tmp_path):
    _refusals(build_driver(), tmp_path)


@pytest.mark.parametrize("tag", ["sq_blast", "pairwise", "split_zip"])
def test_ziprows_device_on_the_kernel_emulator(tag, tmp_path):
    _case(_emu_driver(), tmp_path, tag)


def test_ziprows_device_refusals_on_the_kernel_emulator(tmp_path):
    _refusals(_emu_driver(), tmp_path)
