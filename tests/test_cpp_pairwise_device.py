"""The C++ host driver (examples/smr_align.cpp) with --pairwise device: the reads file is uploaded with SMR_FASTX_KEEP and the BLAST pairwise text
of --blast 0 comes from one smr_pairwise_part call per (index, part) + smr_report_add_pairwise instead of smr_reads_record_text + smr_report_add
read by read.  Every file the run writes must be byte-identical to the --pairwise host run's (both with --pack device) -- except where a file
quotes the run's own command line, left out the way test_cpp_split_device.py leaves it out."""
import os
import subprocess

import pytest

from helpers import golden
from test_cpp_driver import _emu_driver, build_driver
from test_cpp_rows_device import _two_db_args
from test_cpp_split_device import _content, _fasta_args, _files, _interleaved_args


def _same_outputs(exe, args, tmp_path, tag, reports=(), device=()):
    """the run with --pairwise host (and none of the `device` switches) against the run with --pairwise device and all of them"""
    outs = {}
    for where, extra in (("host", ["--pairwise", "host"]), ("device", ["--pairwise", "device"] + list(device))):
        outs[where] = tmp_path / (tag + "_" + where)
        os.makedirs(outs[where])
        subprocess.check_call([exe] + args + ["--blast", "0"] + list(reports) + extra + ["--out", str(outs[where]), "--pack", "device"])
    fa = _files(outs["host"])
    assert fa == _files(outs["device"]) and "aligned.blast" in fa, tag
    differ = [f for f in fa if _content(str(outs["host"] / f)) != _content(str(outs["device"] / f))]
    assert not differ, (tag, differ)
    assert _content(str(outs["device"] / "aligned.blast")).count(b"Sequence ID: ") > 3, "%s: aligned.blast holds no blocks: the comparison shows nothing" % tag
    if "--sam" in reports:
        assert _content(str(outs["device"] / "aligned.sam")).count(b"\n") > 3, tag


def _case(exe, tmp_path, tag):
    one = _fasta_args("syn_default")
    if tag == "blast0":
        _same_outputs(exe, one, tmp_path, tag)
    elif tag == "sam_rows":                                # SAM from smr_rows_part next to it
        _same_outputs(exe, one, tmp_path, tag, ["--sam", "-SQ"], device=["--rows", "device"])
    elif tag == "two_db":                                  # several (index, part): each part is uploaded again for its text
        _same_outputs(exe, _two_db_args(), tmp_path, tag, ["--sam"], device=["--rows", "device"])
    else:                                                  # interleaved mates and --split device: the per-read loop feeds the report nothing
        _same_outputs(exe, _interleaved_args(tmp_path) + ["-paired_in"], tmp_path, tag, ["--sam", "--fastx", "--other"], device=["--rows", "device", "--split", "device"])


CASES = ["blast0", "sam_rows", "two_db", "interleaved_split"]


def _refusals(exe, tmp_path):
    one = _fasta_args("syn_default")
    run = lambda args: subprocess.run([exe] + args + ["--out", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    p = run(one + ["--pairwise", "device", "--blast", "0"])
    assert p.returncode != 0 and b"--pack device" in p.stderr
    p = run(one + ["--pack", "device", "--pairwise", "device", "--sam"])
    assert p.returncode != 0 and b"--blast 0" in p.stderr
    p = run(one + ["--reads", golden.inputs("syn_default")[1], "--pack", "device", "--pairwise", "device", "--blast", "0"])
    assert p.returncode != 0 and b"one reads file" in p.stderr
    p = run(one + ["--pack", "device", "--rows", "device", "--pairwise", "host", "--blast", "0"])      # without the switch --rows device goes on refusing --blast 0
    assert p.returncode != 0 and b"--blast 0" in p.stderr
    assert not os.listdir(str(tmp_path))                                  # refused before anything was loaded or written


@pytest.mark.gpu
@pytest.mark.parametrize("tag", CASES)
def test_pairwise_device_gives_the_files_of_pairwise_host(tag, tmp_path):
    _case(build_driver(), tmp_path, tag)


@pytest.mark.gpu
def test_pairwise_device_refusals(tmp_path):
    _refusals(build_driver(), tmp_path)


@pytest.mark.parametrize("tag", CASES)
def test_pairwise_device_on_the_kernel_emulator(tag, tmp_path):
    _case(_emu_driver(), tmp_path, tag)


def test_pairwise_device_refusals_on_the_kernel_emulator(tmp_path):
    _refusals(_emu_driver(), tmp_path)
