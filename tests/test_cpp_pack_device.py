"""The C++ host driver (examples/smr_align.cpp) with --pack device: the reads files go through smr_reads_upload_fastx_file (parsed and packed
by kernels) instead of smr_reads_load_fastx_text + smr_reads_upload.  Every file the run writes must be byte-identical to the --pack host
run's -- except where a file quotes the run's own command line, which names --pack and --out: the @PG line of aligned.sam, and in aligned.log
the command line at its head and the time stamp at its foot (left out the way test_cpp_driver.py leaves them out)."""
import json
import os
import subprocess

import pytest

from helpers import golden, paths
from test_cpp_driver import _emu_driver, build_driver

REPORTS = ["--fastx", "--other", "--blast", "1 cigar qcov qstrand", "--sam"]


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def _content(path):
    data = open(path, "rb").read()
    if path.endswith("aligned.sam"):
        return b"\n".join(l for l in data.split(b"\n") if not l.startswith(b"@PG"))
    if path.endswith("aligned.log"):
        return b"\n".join(data.split(b"\n")[3:-3])
    return data


def _same_outputs(exe, args, tmp_path):
    outs = {}
    for pack in ("host", "device"):
        outs[pack] = tmp_path / pack
        os.makedirs(outs[pack])
        subprocess.check_call([exe] + args + REPORTS + ["--out", str(outs[pack]), "--pack", pack])
    fa = _files(outs["host"])
    assert fa == _files(outs["device"])
    for want in ("aligned.blast", "aligned.sam", "records.bin", "summary.txt", "aligned.log"):
        assert want in fa, (want, fa)
    assert any(f.startswith(("aligned.f", "aligned_fwd.f")) for f in fa) and any(f.startswith(("other.f", "other_fwd.f")) for f in fa), fa
    differ = [f for f in fa if _content(str(outs["host"] / f)) != _content(str(outs["device"] / f))]
    assert not differ, differ
    assert any(not l.startswith("@") for l in open(outs["device"] / "aligned.sam")), "no read aligned: the comparison shows nothing"


def _fasta_args(case):
    g = golden.load()[case]
    db, rd, _ = golden.inputs(case)
    return ["--reads", rd, "--ref", db, "--gumbel", repr(g["log"]["lambda"][0]), repr(g["log"]["K"][0])]


def _paired_args():
    pd = os.path.join(paths.REPO, "tests", "golden", "paired")
    log = json.load(open(os.path.join(pd, "paired.json")))["two_files"]["log"]
    db = os.path.join(paths.REPO, "tests", "golden", "real_db.fasta")
    return ["--ref", db, "--gumbel", repr(log["lambda"][0]), repr(log["K"][0]), "--reads", os.path.join(pd, "paired_1.fastq"), "--reads", os.path.join(pd, "paired_2.fastq"),
            "-paired_in", "-out2"]


@pytest.mark.gpu
def test_pack_device_gives_the_files_of_pack_host_fasta(tmp_path):
    _same_outputs(build_driver(), _fasta_args("syn_default"), tmp_path)


@pytest.mark.gpu
def test_pack_device_gives_the_files_of_pack_host_paired_fastq(tmp_path):
    exe = build_driver()
    _same_outputs(exe, _paired_args(), tmp_path)
    p = subprocess.run([exe, "--pack", "sometimes"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)          # refused before anything runs
    assert p.returncode != 0 and b"--pack" in p.stderr


def test_pack_device_on_the_kernel_emulator_fasta(tmp_path):
    _same_outputs(_emu_driver(), _fasta_args("real_default"), tmp_path)


def test_pack_device_on_the_kernel_emulator_paired_fastq(tmp_path):
    _same_outputs(_emu_driver(), _paired_args(), tmp_path)
