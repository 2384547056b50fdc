"""The C++ host driver (examples/smr_align.cpp) with --unzip device: a gzip reads file is handed to smr_reads_upload_fastx_file under
SMR_FASTX_INFLATE, i.e. inflated by the DEFLATE decoder kernels instead of by zlib on the host.  The run must write the files of the
--unzip host run (both with --pack device), compared the way test_cpp_split_device.py compares them: gzip files by what they inflate to, and
without the lines that quote the run's own command line."""
import gzip
import os
import subprocess

import pytest

from helpers import golden
from test_cpp_driver import _emu_driver, build_driver
from test_cpp_split_device import _content, _files, _paired_base

REPORTS = ["--fastx", "--other", "--blast", "1 cigar qcov qstrand", "--sam"]


def _gz(src, dst):
    with open(src, "rb") as f, gzip.open(dst, "wb", 6) as g:
        g.write(f.read())
    return dst


def _same_outputs(exe, args, tmp_path, tag, extra=()):
    outs = {}
    for unzip in ("host", "device"):
        outs[unzip] = tmp_path / (tag + "_" + unzip)
        os.makedirs(outs[unzip])
        subprocess.check_call([exe] + args + REPORTS + list(extra) + ["--out", str(outs[unzip]), "--pack", "device", "--unzip", unzip])
    fa = _files(outs["host"])
    assert fa == _files(outs["device"]), tag
    fx = [f for f in fa if f.startswith("aligned") and ".f" in f and f.endswith(".gz")]
    assert fx, (tag, fa)                                   # (a gzip reads file: gzip reports)
    differ = [f for f in fa if _content(str(outs["host"] / f)) != _content(str(outs["device"] / f))]
    assert not differ, (tag, differ)
    assert sum(len(_content(str(outs["device"] / f))) for f in fx) > 0, "no read aligned: the comparison shows nothing"


def _fastq(exe, tmp_path, single=True):
    pd, base = _paired_base()
    reads = [_gz(os.path.join(pd, "paired_%d.fastq" % k), str(tmp_path / ("paired_%d.fq.gz" % k))) for k in (1, 2)]
    if single:
        _same_outputs(exe, base + ["--reads", reads[0]], tmp_path, "single")
    _same_outputs(exe, base + ["--reads", reads[0], "--reads", reads[1], "-paired_out", "-out2"], tmp_path, "two_files", extra=["--split", "device"])


def _fasta(exe, case, tmp_path):
    g = golden.load()[case]
    db, rd, _ = golden.inputs(case)
    reads = _gz(rd, str(tmp_path / "reads.fa.gz"))
    _same_outputs(exe, ["--reads", reads, "--ref", db, "--gumbel", repr(g["log"]["lambda"][0]), repr(g["log"]["K"][0])], tmp_path, "fasta")


def _refusals(exe):
    db, rd, _ = golden.inputs("syn_default")
    base = [exe, "--ref", db, "--gumbel", "0.6", "0.33", "--reads", rd]
    p = subprocess.run(base + ["--unzip", "device"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)       # refused before anything is loaded
    assert p.returncode != 0 and b"--unzip device" in p.stderr and b"--pack device" in p.stderr, p.stderr
    p = subprocess.run(base + ["--pack", "host", "--unzip", "device"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--pack device" in p.stderr, p.stderr
    p = subprocess.run(base + ["--unzip", "sometimes"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--unzip" in p.stderr, p.stderr
    assert "--unzip host|device" in subprocess.check_output([exe, "--help"]).decode()


@pytest.mark.gpu
def test_unzip_device_gives_the_files_of_unzip_host_fastq(tmp_path):
    _fastq(build_driver(), tmp_path)


@pytest.mark.gpu
def test_unzip_device_gives_the_files_of_unzip_host_fasta(tmp_path):
    _fasta(build_driver(), "syn_default", tmp_path)


def test_unzip_device_on_the_kernel_emulator_fastq(tmp_path):
    _fastq(_emu_driver(), tmp_path, single=False)


def test_the_switch_is_refused_before_anything_is_loaded():
    _refusals(build_driver())
