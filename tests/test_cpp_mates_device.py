"""The C++ host driver (examples/smr_align.cpp) with --mates device: two reads files (mates) under --rows device / --pairwise device /
--ziprows device.  The rows and the pairwise text come from smr_rows_part_mates / smr_pairwise_part_mates (and their _gz forms) per (index,
part) instead of smr_reads_record_text + smr_report_add_pair pair by pair.  Every file the run writes must be byte-identical (gzip files:
after inflating) to the files of the same run with --mates host, where the host writer makes the rows -- except where a file quotes the
run's own command line, left out the way test_cpp_split_device.py leaves it out."""
import os
import subprocess

import pytest

from test_cpp_driver import _emu_driver, build_driver
from test_cpp_split_device import _content, _files, _paired_args

BLAST = ["--blast", "1 cigar qcov qstrand"]
CASES = {
    "rows": (["--sam"] + BLAST, ["--rows", "device"]),
    "pairwise": (["--blast", "0"], ["--pairwise", "device"]),
    "ziprows": (["--sam", "-zip-out", "1"] + BLAST, ["--rows", "device", "--ziprows", "device"]),
    "zip_pairwise": (["--blast", "0", "-zip-out", "1"], ["--pairwise", "device", "--ziprows", "device"]),
    "split": (["--sam", "--fastx", "--other", "-paired_in", "-out2"] + BLAST, ["--rows", "device", "--split", "device"]),
}


def _case(exe, tmp_path, tag):
    reports, device = CASES[tag]
    outs = {}
    for mates in ("host", "device"):
        outs[mates] = tmp_path / (tag + "_" + mates)
        os.makedirs(outs[mates])
        subprocess.check_call([exe] + _paired_args() + reports + ["--pack", "device", "--mates", mates, "--out", str(outs[mates])] + (device if mates == "device" else []))
    fa = _files(outs["host"])
    assert fa == _files(outs["device"]), tag
    differ = [f for f in fa if _content(str(outs["host"] / f)) != _content(str(outs["device"] / f))]
    assert not differ, (tag, differ)
    gz = ".gz" if "-zip-out" in reports else ""
    for f, flag in (("aligned.sam" + gz, "--sam"), ("aligned.blast" + gz, "--blast")):
        if flag in reports:
            assert f in fa and _content(str(outs["device"] / f)).count(b"\n") > 100, "%s: %s holds no rows: the comparison shows nothing" % (tag, f)


def _refusals(exe, tmp_path):
    two = _paired_args()
    one = two[:-2]
    run = lambda args: subprocess.run([exe] + args + ["--out", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)      # noqa: E731
    p = run(one + ["--pack", "device", "--rows", "device", "--mates", "device", "--sam"])
    assert p.returncode != 0 and b"--mates device" in p.stderr and b"two --reads files" in p.stderr
    p = run(two + ["--pack", "device", "--mates", "device", "--sam"])
    assert p.returncode != 0 and b"--mates device" in p.stderr and b"--rows device" in p.stderr and b"--pairwise device" in p.stderr
    p = run(two + ["--pack", "device", "--rows", "device", "--mates", "device", "--sam", "-otu_map", "--otu", "device"])
    assert p.returncode != 0 and b"--otu device takes one reads file" in p.stderr
    p = run(two + ["--pack", "device", "--rows", "device", "--mates", "bogus", "--sam"])
    assert p.returncode != 0 and b"--mates: host or device" in p.stderr
    # without the switch, and with --mates host, the refusals of two reads files are what they were
    for extra in ([], ["--mates", "host"]):
        p = run(two + ["--pack", "device", "--rows", "device", "--sam"] + extra)
        assert p.returncode != 0 and b"--rows device takes one reads file" in p.stderr
        p = run(two + ["--pack", "device", "--pairwise", "device", "--blast", "0"] + extra)
        assert p.returncode != 0 and b"--pairwise device takes one reads file" in p.stderr
    assert not os.listdir(str(tmp_path))                                  # refused before anything was loaded or written


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_mates_device_gives_the_files_of_mates_host(tag, tmp_path):
    _case(build_driver(), tmp_path, tag)


@pytest.mark.gpu
def test_mates_device_refusals(tmp_path):
    _refusals(build_driver(), tmp_path)


@pytest.mark.parametrize("tag", ["rows", "pairwise", "ziprows", "split"])
def test_mates_device_on_the_kernel_emulator(tag, tmp_path):
    _case(_emu_driver(), tmp_path, tag)


def test_mates_device_refusals_on_the_kernel_emulator(tmp_path):
    _refusals(_emu_driver(), tmp_path)
