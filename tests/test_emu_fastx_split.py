"""The bodies of test_gpu_fastx_split.py on the emulator (the kernel sources compiled for the host, tests/emu): the measure, scan and copy
kernels of csrc/smr_fxsplit.hpp without a GPU.  Same bodies, another library behind the binding; device memory lies between guard pages
there, so a load behind the padded text or a store behind the last record's last byte faults at once."""
import pytest

from helpers import emu
from test_gpu_fastx_device import DRESSINGS, SCAN_COUNTS
from test_gpu_fastx_split import OWN_HITS_CASES, boundaries_body, guards_body, irregular_body, long_body, own_hits_body, pairs_body, scan_body


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.mark.parametrize("how", DRESSINGS)
@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_boundaries(fastq, how, tmp_path):
    boundaries_body(fastq, how, tmp_path)


@pytest.mark.parametrize("n_rec", SCAN_COUNTS)
@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_scans(fastq, n_rec, tmp_path):
    scan_body(fastq, n_rec, tmp_path)


@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_a_header_and_a_record_longer_than_a_team_copies(fastq, tmp_path):
    long_body(fastq, tmp_path)


def test_pairs_under_every_option_set(tmp_path):
    pairs_body(tmp_path)


def test_irregular_text_with_keep(tmp_path):
    irregular_body(tmp_path)


@pytest.mark.parametrize("case", OWN_HITS_CASES)
def test_the_batchs_own_hits(case, tmp_path):
    own_hits_body(case, tmp_path)


def test_guards(tmp_path):
    guards_body(tmp_path)
