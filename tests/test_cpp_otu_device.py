"""The C++ host driver (examples/smr_align.cpp) under -otu_map -de_novo_otu with --otu device: the members of otu_map.txt come from one
smr_otu_part call per (index, part) + smr_report_add_otu and aligned_denovo.* from one smr_fastx_denovo call + smr_report_add_denovo, instead of
smr_report_add read by read.  Every file the run writes must be byte-identical to the --otu host run's (the device run with the other device
switches on as well, so that its per-read loop feeds the report nothing) -- except where a file quotes the run's own command line, left out the
way test_cpp_split_device.py leaves it out -- and otu_map.txt / aligned_denovo.fa must be the files the unmodified reference wrote
(tests/golden/otu/)."""
import os
import subprocess

import pytest

from helpers import golden, otu, paths
from test_cpp_driver import _emu_driver, build_driver
from test_cpp_split_device import ROWS, _content, _files

DEVICE = ["--split", "device", "--rows", "device", "--otu", "device"]


def _args(case):
    g = otu.load()[case]
    gg = golden.load()[g["inputs"]]
    dbs, rd, _ = golden.inputs(g["inputs"])
    a = ["--reads", rd]
    for k, db in enumerate(dbs if isinstance(dbs, list) else [dbs]):
        a += ["--ref", db, "--gumbel", repr(gg["log"]["lambda"][k]), repr(gg["log"]["K"][k])]
    return a + ["-otu_map", "-de_novo_otu", "-id", repr(g["min_id"]), "-coverage", repr(g["min_cov"])]


def _same_outputs(exe, case, tmp_path, reports=("--fastx", "--other") + tuple(ROWS)):
    g = otu.load()[case]
    outs = {}
    for mode, switches in (("host", ["--otu", "host"]), ("device", DEVICE)):
        outs[mode] = tmp_path / (case + "_" + mode)
        os.makedirs(outs[mode])
        subprocess.check_call([exe] + _args(case) + list(reports) + ["--out", str(outs[mode]), "--pack", "device"] + switches)
    fa = _files(outs["host"])
    assert fa == _files(outs["device"]), case
    assert "aligned_denovo.fa" in fa and "records.bin" in fa and ("otu_map.txt" in fa) == (g["otu_map"] is not None), fa
    differ = [f for f in fa if _content(str(outs["host"] / f)) != _content(str(outs["device"] / f))]
    assert not differ, (case, differ)
    for mode in outs:
        if g["otu_map"]:
            assert open(outs[mode] / "otu_map.txt", "rb").read() == open(os.path.join(otu.OTU_DIR, g["otu_map"]), "rb").read(), (case, mode)
        assert open(outs[mode] / "aligned_denovo.fa", "rb").read() == open(os.path.join(otu.OTU_DIR, case + ".denovo.fa"), "rb").read(), (case, mode)
        log = open(outs[mode] / "aligned.log").read()
        assert "Total reads for de novo clustering = %d" % g["totals"][3] in log and "Total OTUs = %d" % g["n_groups"] in log, (case, mode)
        assert "num_yid_ycov = %d\n" % g["totals"][0] in open(outs[mode] / "summary.txt").read()


def _refusals(exe):
    db, rd, _ = golden.inputs("syn_default")
    base = [exe, "--ref", db, "--gumbel", "0.6", "0.33"]
    for extra, word in ((["--reads", rd, "-otu_map", "--otu", "device"], "--pack device"),                         # no --pack device
                        (["--reads", rd, "--reads", rd, "-otu_map", "--pack", "device", "--otu", "device"], "one reads file"),      # two reads files
                        (["--reads", rd, "-id", "0.9"], "-otu_map"),                                               # -id without -otu_map
                        (["--reads", rd, "--otu", "sometimes"], "--otu")):
        p = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE)          # refused before anything is loaded
        assert p.returncode != 0 and word.encode() in p.stderr, (extra, p.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["syn", "two_db"])
def test_otu_device_gives_the_files_of_otu_host_and_of_the_reference(case, tmp_path):
    _same_outputs(build_driver(), case, tmp_path)


def test_the_switch_is_refused_before_anything_is_loaded():
    _refusals(build_driver())


def test_otu_device_on_the_kernel_emulator(tmp_path):
    _same_outputs(_emu_driver(), "syn", tmp_path)
