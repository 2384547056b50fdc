"""The bodies of test_gpu_pairwise.py on the emulator (the kernel sources compiled for the host, tests/emu): k_rows_stat's guards, k_pair_size and
k_pair_write without a GPU.  Same bodies, another library behind the binding; device memory lies between guard pages there, so a store behind
the last block's last byte faults at once."""
import pytest

from helpers import emu
from test_gpu_pairwise import COUNTS, FIXTURES, WORKLOADS, columns_body, contract_body, crafted_body, fixture_body, n_reference_body, workload_body


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


def test_explicit_cigars_equal_the_host_writer(tmp_path):
    columns_body(tmp_path)


def test_a_reference_with_n_equals_the_host_writer(tmp_path):
    n_reference_body(tmp_path)


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("n", COUNTS)
def test_crafted_state_equals_the_host_writer(n, fastq, tmp_path):
    crafted_body(n, fastq, tmp_path, seed=n)


def test_a_block_longer_than_the_window_next_to_short_blocks(tmp_path):
    crafted_body(70, True, tmp_path, seed=5, long_read=True)


@pytest.mark.parametrize("case", WORKLOADS)
def test_workload_text_equals_the_host_loop(case, tmp_path):
    workload_body(case, tmp_path)


@pytest.mark.parametrize("case", FIXTURES)
def test_the_device_text_equals_the_reference_file(case, tmp_path):
    fixture_body(case, tmp_path)


def test_contract_and_refusals(tmp_path):
    contract_body(tmp_path)
