"""The C++ host driver (examples/smr_align.cpp) with --rows device: the reads file is uploaded with SMR_FASTX_KEEP and the rows of aligned.sam
and of the BLAST tabular report come from one smr_rows_part call per (index, part) + smr_report_add_rows instead of smr_reads_record_text +
smr_report_add read by read.  Every file the run writes must be byte-identical to the --rows host run's (both with --pack device) -- except
where a file quotes the run's own command line, left out the way test_cpp_split_device.py leaves it out."""
import os
import subprocess

import pytest

from helpers import golden
from test_cpp_driver import _emu_driver, build_driver
from test_cpp_split_device import _content, _fasta_args, _files, _interleaved_args

BLAST = ["--blast", "1 cigar qcov qstrand"]


def _same_outputs(exe, args, tmp_path, tag, reports, extra=()):
    outs = {}
    for rows in ("host", "device"):
        outs[rows] = tmp_path / (tag + "_" + rows)
        os.makedirs(outs[rows])
        subprocess.check_call([exe] + args + list(reports) + list(extra) + ["--out", str(outs[rows]), "--pack", "device", "--rows", rows])
    fa = _files(outs["host"])
    assert fa == _files(outs["device"]), tag
    differ = [f for f in fa if _content(str(outs["host"] / f)) != _content(str(outs["device"] / f))]
    assert not differ, (tag, differ)
    for f, flag in (("aligned.sam", "--sam"), ("aligned.blast", "--blast")):
        if flag in reports:
            assert _content(str(outs["device"] / f)).count(b"\n") > 3, "%s: %s holds no rows: the comparison shows nothing" % (tag, f)


def _two_db_args():
    g = golden.load()["two_db_default"]
    dbs, rd, _ = golden.inputs("two_db_default")
    args = ["--reads", rd]
    for k, db in enumerate(dbs):
        args += ["--ref", db, "--gumbel", repr(g["log"]["lambda"][k]), repr(g["log"]["K"][k])]
    return args


def _case(exe, tmp_path, tag):
    one = _fasta_args("syn_default")
    if tag == "sam":
        _same_outputs(exe, one, tmp_path, tag, ["--sam"])
    elif tag == "blast":
        _same_outputs(exe, one, tmp_path, tag, BLAST)
    elif tag == "sq":
        _same_outputs(exe, one, tmp_path, tag, ["--sam", "-SQ"] + BLAST)
    elif tag == "all":
        _same_outputs(exe, one + ["-num_alignments", "0", "-no-best"], tmp_path, tag, ["--sam"] + BLAST)
    elif tag == "two_db":                                  # several (index, part): each part is uploaded again for its rows
        _same_outputs(exe, _two_db_args(), tmp_path, tag, ["--sam"] + BLAST)
    elif tag == "interleaved":
        _same_outputs(exe, _interleaved_args(tmp_path) + ["-paired_out"], tmp_path, tag, ["--sam", "--fastx", "--other"] + BLAST)
    elif tag == "split":
        _same_outputs(exe, one, tmp_path, tag, ["--sam", "--fastx", "--other"] + BLAST, extra=["--split", "device"])
    else:                                                  # interleaved mates and --split device together: the per-read loop feeds the report nothing
        _same_outputs(exe, _interleaved_args(tmp_path) + ["-paired_in"], tmp_path, tag, ["--sam", "-SQ", "--fastx", "--other"] + BLAST, extra=["--split", "device"])


CASES = ["sam", "blast", "sq", "all", "two_db", "interleaved", "split", "interleaved_split"]


def _refusals(exe, tmp_path):
    one = _fasta_args("syn_default")
    p = subprocess.run([exe] + one + ["--pack", "device", "--rows", "device", "--blast", "0", "--out", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--blast 0" in p.stderr
    rd = golden.inputs("syn_default")[1]
    p = subprocess.run([exe] + one + ["--reads", rd, "--pack", "device", "--rows", "device", "--sam", "--out", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"one reads file" in p.stderr
    p = subprocess.run([exe] + one + ["--rows", "device", "--sam"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--pack device" in p.stderr
    assert not os.listdir(str(tmp_path))                                  # refused before anything was loaded or written


@pytest.mark.gpu
@pytest.mark.parametrize("tag", CASES)
def test_rows_device_gives_the_files_of_rows_host(tag, tmp_path):
    _case(build_driver(), tmp_path, tag)


@pytest.mark.gpu
def test_rows_device_refusals(tmp_path):
    _refusals(build_driver(), tmp_path)


@pytest.mark.parametrize("tag", ["sq", "two_db", "interleaved_split"])
def test_rows_device_on_the_kernel_emulator(tag, tmp_path):
    _case(_emu_driver(), tmp_path, tag)


def test_rows_device_refusals_on_the_kernel_emulator(tmp_path):
    _refusals(_emu_driver(), tmp_path)
