"""The C++ host driver (examples/smr_align.cpp) with --otu-mates device: two reads files (mates) under -otu_map -de_novo_otu.  The members of
otu_map.txt come from smr_otu_part_mates per (index, part) and aligned_denovo.* from one smr_fastx_denovo call of layout 2, instead of
smr_reads_record_text + smr_report_add_pair pair by pair.  Every file the run writes must be byte-identical to the files of the same run
without the switch, where the host writer makes them -- except where a file quotes the run's own command line, left out the way
test_cpp_split_device.py leaves it out.  The thresholds are the loose ones of the paired_loose fixture: under them the map holds a member (a
second mate); under the defaults no read of the fixture passes and no map is written."""
import os
import subprocess

import pytest

from test_cpp_driver import _emu_driver, build_driver
from test_cpp_split_device import _content, _files, _paired_args

OTU = ["-otu_map", "-de_novo_otu", "-id", "0.9", "-coverage", "0.5"]
BLAST = ["--blast", "1 cigar qcov qstrand"]
# reports of the run, switches of the default run, switches of the device run
CASES = {
    "plain": (["--fastx", "--other"], ["--split", "device"], ["--split", "device", "--otu-mates", "device"]),
    "rows": (["--fastx", "--other", "--sam"] + BLAST, ["--split", "device"], ["--split", "device", "--mates", "device", "--rows", "device", "--otu-mates", "device"]),
    "out2": (["--fastx", "--other", "-paired_in", "-out2"], ["--split", "device"], ["--split", "device", "--otu-mates", "device"]),
}


def _case(exe, tmp_path, tag):
    reports, host, device = CASES[tag]
    outs = {}
    for mode, extra in (("host", host), ("device", device)):
        outs[mode] = tmp_path / (tag + "_" + mode)
        os.makedirs(outs[mode])
        subprocess.check_call([exe] + _paired_args() + OTU + reports + ["--pack", "device", "--out", str(outs[mode])] + extra)
    fa = _files(outs["host"])
    assert fa == _files(outs["device"]), tag
    differ = [f for f in fa if _content(str(outs["host"] / f)) != _content(str(outs["device"] / f))]
    assert not differ, (tag, differ)
    assert "otu_map.txt" in fa and open(outs["device"] / "otu_map.txt", "rb").read().count(b"\t") >= 1, "%s: the map holds no member: the comparison shows nothing" % tag
    dn = [f for f in fa if f.startswith("aligned_denovo")]
    assert dn and sum(os.path.getsize(outs["device"] / f) for f in dn) > 0, tag
    assert len(dn) == (2 if tag == "out2" else 1), dn


def _refusals(exe, tmp_path):
    two = _paired_args()
    one = two[:-2]
    run = lambda args: subprocess.run([exe] + args + ["--out", str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)      # noqa: E731
    p = run(one + ["--pack", "device", "--otu-mates", "device"] + OTU)
    assert p.returncode != 0 and b"--otu-mates device" in p.stderr and b"two --reads files" in p.stderr
    p = run(two + ["--otu-mates", "device"] + OTU)
    assert p.returncode != 0 and b"--otu-mates device" in p.stderr and b"--pack device" in p.stderr
    p = run(two + ["--pack", "device", "--otu-mates", "bogus"] + OTU)
    assert p.returncode != 0 and b"--otu-mates: host or device" in p.stderr
    # --otu device with two files is refused in its old words, with and without the new switch
    for extra in ([], ["--otu-mates", "host"], ["--otu-mates", "device"]):
        p = run(two + ["--pack", "device", "--otu", "device"] + OTU + extra)
        assert p.returncode != 0 and (b"--otu device takes one reads file (single reads or interleaved mates): the members of a group of mates in two files alternate "
                                      b"between the batches and stay with --otu host") in p.stderr
    assert not os.listdir(str(tmp_path))                                  # refused before anything was loaded or written


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(CASES))
def test_otu_mates_device_gives_the_files_of_the_default_run(tag, tmp_path):
    _case(build_driver(), tmp_path, tag)


@pytest.mark.gpu
def test_otu_mates_device_refusals(tmp_path):
    _refusals(build_driver(), tmp_path)


@pytest.mark.parametrize("tag", ["plain", "rows", "out2"])
def test_otu_mates_device_on_the_kernel_emulator(tag, tmp_path):
    _case(_emu_driver(), tmp_path, tag)


def test_otu_mates_device_refusals_on_the_kernel_emulator(tmp_path):
    _refusals(_emu_driver(), tmp_path)
