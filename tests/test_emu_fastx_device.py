"""The bodies of test_gpu_fastx_device.py on the emulator (the kernel sources compiled for the host, tests/emu): the line, record and pack
kernels of csrc/smr_fastx.hpp without a GPU.  Same bodies, another library behind the binding; device memory lies between guard pages there,
so a load behind the padded text or a store behind the batch's last word faults at once."""
import pytest

from helpers import emu
from test_gpu_fastx_device import DRESSINGS, GOLDEN_CASES, SCAN_COUNTS, boundaries_body, golden_body, guards_body, irregular_body, long_body, scan_body


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.mark.parametrize("how", DRESSINGS)
@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_packing_at_its_boundaries(fastq, how, tmp_path):
    boundaries_body(fastq, how, tmp_path)


@pytest.mark.parametrize("n_rec", SCAN_COUNTS)
@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_scan_boundaries(fastq, n_rec, tmp_path):
    scan_body(fastq, n_rec, tmp_path)


@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_a_header_and_a_record_longer_than_a_tile(fastq, tmp_path):
    long_body(fastq, tmp_path)


def test_irregular_and_malformed_text(tmp_path):
    irregular_body(tmp_path)


@pytest.mark.parametrize("case,how", GOLDEN_CASES)
def test_the_batch_is_the_uploaded_one(case, how, tmp_path):
    golden_body(case, how, tmp_path)


def test_guards(tmp_path):
    guards_body(tmp_path)
