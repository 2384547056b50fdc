"""The C++ host driver (examples/smr_align.cpp) with --split device: the reads files are uploaded with SMR_FASTX_KEEP and aligned.* / other.*
come from one smr_fastx_split call + smr_report_add_fastx instead of smr_reads_record_text + smr_report_add / _add_pair read by read.  Every
file the run writes must be byte-identical to the --split host run's (both with --pack device) -- except where a file quotes the run's own
command line, left out the way test_cpp_pack_device.py leaves it out; gzip files are compared by what they inflate to."""
import gzip
import json
import os
import subprocess

import pytest

from helpers import golden, paths
from test_cpp_driver import _emu_driver, build_driver

ROWS = ["--blast", "1 cigar qcov qstrand", "--sam"]


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _content(path):
    data = gzip.open(path, "rb").read() if path.endswith(".gz") else open(path, "rb").read()
    name = path[:-3] if path.endswith(".gz") else path
    if name.endswith("aligned.sam"):
        return b"\n".join(l for l in data.split(b"\n") if not l.startswith(b"@PG"))
    if name.endswith("aligned.log"):
        return b"\n".join(data.split(b"\n")[3:-3])
    return data


def _same_outputs(exe, args, tmp_path, tag, reports=("--fastx", "--other") + tuple(ROWS)):
    outs = {}
    for split in ("host", "device"):
        outs[split] = tmp_path / (tag + "_" + split)
        os.makedirs(outs[split])
        subprocess.check_call([exe] + args + list(reports) + ["--out", str(outs[split]), "--pack", "device", "--split", split])
    fa = _files(outs["host"])
    assert fa == _files(outs["device"]), tag
    assert any(f.startswith("aligned") and ".f" in f for f in fa) and any(f.startswith("other") and ".f" in f for f in fa), (tag, fa)
    differ = [f for f in fa if _content(str(outs["host"] / f)) != _content(str(outs["device"] / f))]
    assert not differ, (tag, differ)
    fx = [f for f in fa if f.startswith(("aligned", "other")) and ".f" in f]
    assert sum(len(_content(str(outs["device"] / f))) for f in fx if f.startswith("aligned")) > 0, "no read aligned: the comparison shows nothing"
    assert sum(len(_content(str(outs["device"] / f))) for f in fx if f.startswith("other")) > 0, "every read aligned: the comparison shows nothing"


def _fasta_args(case):
    g = golden.load()[case]
    db, rd, _ = golden.inputs(case)
    return ["--reads", rd, "--ref", db, "--gumbel", repr(g["log"]["lambda"][0]), repr(g["log"]["K"][0])]


def _paired_base():
    pd = os.path.join(paths.REPO, "tests", "golden", "paired")
    log = json.load(open(os.path.join(pd, "paired.json")))["two_files"]["log"]
    db = os.path.join(paths.REPO, "tests", "golden", "real_db.fasta")
    return pd, ["--ref", db, "--gumbel", repr(log["lambda"][0]), repr(log["K"][0])]


def _paired_args():
    pd, base = _paired_base()
    return base + ["--reads", os.path.join(pd, "paired_1.fastq"), "--reads", os.path.join(pd, "paired_2.fastq")]


def _interleaved_args(tmp_path):
    pd, base = _paired_base()
    inter = str(tmp_path / "interleaved.fastq")
    a, b = open(os.path.join(pd, "paired_1.fastq")).readlines(), open(os.path.join(pd, "paired_2.fastq")).readlines()
    with open(inter, "w") as f:
        for i in range(len(a) // 4):
            f.writelines(a[4 * i:4 * i + 4])
            f.writelines(b[4 * i:4 * i + 4])
    return base + ["--reads", inter]


def _fasta(exe, case, tmp_path):
    _same_outputs(exe, _fasta_args(case), tmp_path, "rows")
    _same_outputs(exe, _fasta_args(case), tmp_path, "fastx_only", reports=("--fastx", "--other"))       # the loop then reads no record text
    _same_outputs(exe, _fasta_args(case) + ["-zip-out", "1"], tmp_path, "zip")


def _paired(exe, tmp_path):
    for tag, flags in [("paired_in", ["-paired_in"]), ("paired_out_out2", ["-paired_out", "-out2"]), ("sout_out2", ["-sout", "-out2"])]:
        _same_outputs(exe, _paired_args() + flags, tmp_path, tag)
    _same_outputs(exe, _interleaved_args(tmp_path) + ["-paired_out"], tmp_path, "interleaved", reports=("--fastx", "--other"))


@pytest.mark.gpu
def test_split_device_gives_the_files_of_split_host_fasta(tmp_path):
    _fasta(build_driver(), "syn_default", tmp_path)


@pytest.mark.gpu
def test_split_device_gives_the_files_of_split_host_paired_fastq(tmp_path):
    exe = build_driver()
    _paired(exe, tmp_path)
    p = subprocess.run([exe, "--split", "device", "--pack", "host"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)          # refused before anything runs
    assert p.returncode != 0 and b"--pack device" in p.stderr
    p = subprocess.run([exe, "--split", "sometimes"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--split" in p.stderr


def test_split_device_on_the_kernel_emulator_fasta(tmp_path):
    _fasta(_emu_driver(), "real_default", tmp_path)


def test_split_device_on_the_kernel_emulator_paired_fastq(tmp_path):
    exe = _emu_driver()
    _paired(exe, tmp_path)
    p = subprocess.run([exe, "--split", "device", "--pack", "host"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--pack device" in p.stderr
