"""The C++ host driver (examples/smr_align.cpp) with --zip device: under gzipped reports aligned.* / other.* come from smr_fastx_split_gz +
smr_report_add_fastx_gz, and with --otu device aligned_denovo.* from smr_fastx_denovo_gz + smr_report_add_denovo_gz -- gzip members made by the
DEFLATE kernels and appended as they are.  The run must write the files of the --zip host run, each equal after inflation (Python's gzip is the
yardstick, and reads the multi-member files the way any downstream tool has to)."""
import os
import subprocess

import pytest

from helpers import golden
from test_cpp_driver import _emu_driver, build_driver
from test_cpp_otu_device import _args as _otu_args
from test_cpp_split_device import _content, _fasta_args, _files, _paired_args

BASE = ["--pack", "device", "--split", "device", "-zip-out", "1"]


def _same_outputs(exe, args, tmp_path, tag, extra=(), expect=("aligned", "other")):
    outs = {}
    for zip_ in ("host", "device"):
        outs[zip_] = tmp_path / (tag + "_" + zip_)
        os.makedirs(outs[zip_])
        subprocess.check_call([exe] + args + ["--fastx", "--other", "--out", str(outs[zip_])] + BASE + list(extra) + ["--zip", zip_])
    fa = _files(outs["host"])
    assert fa == _files(outs["device"]), tag
    differ = [f for f in fa if _content(str(outs["host"] / f)) != _content(str(outs["device"] / f))]
    assert not differ, (tag, differ)
    for what in expect:
        fx = [f for f in fa if f.startswith(what + ".") or f.startswith(what + "_") and not (what == "aligned" and f.startswith("aligned_denovo"))]
        fx = [f for f in fx if f.endswith((".fa.gz", ".fq.gz"))]
        assert fx, (tag, what, fa)
        assert sum(len(_content(str(outs["device"] / f))) for f in fx) > 0, "%s: %s is empty: the comparison shows nothing" % (tag, what)
    return outs


def _fasta(exe, case, tmp_path):
    _same_outputs(exe, _fasta_args(case), tmp_path, "fasta")


def _paired(exe, tmp_path):
    _same_outputs(exe, _paired_args() + ["-paired_out", "-out2"], tmp_path, "paired_out_out2")


def _denovo(exe, tmp_path):
    outs = _same_outputs(exe, _otu_args("syn"), tmp_path, "denovo", extra=["--rows", "device", "--otu", "device"], expect=("aligned", "other", "aligned_denovo"))
    assert os.path.isfile(outs["device"] / "aligned_denovo.fa.gz")


def _refusals(exe):
    db, rd, _ = golden.inputs("syn_default")
    base = [exe, "--ref", db, "--gumbel", "0.6", "0.33", "--reads", rd]
    for extra in (["--pack", "device", "-zip-out", "1", "--zip", "device"],                       # without --split device
                  ["--pack", "device", "--split", "device", "-zip-out", "0", "--zip", "device"],  # the reports are not gzipped
                  ["--pack", "device", "--split", "device", "--zip", "device"],                   # nor are they for a plain reads file
                  ["--zip", "sometimes"]):
        p = subprocess.run(base + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE)          # refused before anything is loaded
        assert p.returncode != 0 and b"--zip" in p.stderr, (extra, p.stderr)
    msgs = [subprocess.run(base + x, stdout=subprocess.PIPE, stderr=subprocess.PIPE).stderr for x in
            (["--pack", "device", "-zip-out", "1", "--zip", "device"], ["--pack", "device", "--split", "device", "-zip-out", "0", "--zip", "device"])]
    assert b"--split device" in msgs[0] and b"--split device" not in msgs[1] and msgs[0] != msgs[1]      # each condition has its own message
    assert "--zip host|device" in subprocess.check_output([exe, "--help"]).decode()


@pytest.mark.gpu
def test_zip_device_inflates_to_the_files_of_zip_host_fasta(tmp_path):
    _fasta(build_driver(), "syn_default", tmp_path)


@pytest.mark.gpu
def test_zip_device_inflates_to_the_files_of_zip_host_paired_fastq(tmp_path):
    _paired(build_driver(), tmp_path)


@pytest.mark.gpu
def test_zip_device_inflates_to_the_files_of_zip_host_denovo(tmp_path):
    _denovo(build_driver(), tmp_path)


def test_zip_device_on_the_kernel_emulator_fasta(tmp_path):
    _fasta(_emu_driver(), "real_default", tmp_path)


def test_zip_device_on_the_kernel_emulator_paired_fastq(tmp_path):
    _paired(_emu_driver(), tmp_path)


def test_zip_device_on_the_kernel_emulator_denovo(tmp_path):
    _denovo(_emu_driver(), tmp_path)


def test_the_switch_is_refused_before_anything_is_loaded():
    _refusals(build_driver())
