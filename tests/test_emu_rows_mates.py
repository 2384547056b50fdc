"""The bodies of test_gpu_rows_mates.py on the emulator (the kernel sources compiled for the host, tests/emu): the stages of smr_rows_part /
smr_pairwise_part over two batches and k_mates_zip without a GPU.  Same bodies, another library behind the binding; device memory lies between
guard pages there, so a store behind a buffer's last byte faults at once."""
import pytest

from helpers import emu, matesdev
from test_gpu_state_import import engine


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("n", matesdev.COUNTS)
def test_crafted_mates_equal_the_host_writer(n, fastq, tmp_path):
    matesdev.crafted_body(engine, n, fastq, tmp_path)


def test_a_long_read_in_batch_1_next_to_short_rows_in_batch_0(tmp_path):
    matesdev.crafted_body(engine, 70, True, tmp_path, long_read=True)


def test_the_paired_workload_in_two_batches(tmp_path):
    matesdev.workload_body(engine, tmp_path)


@pytest.mark.parametrize("n,fastq", [(65, False), (1025, True)])
def test_gz_forms_are_the_plain_bytes_cut_at_line_ends(n, fastq):
    matesdev.gz_body(engine, n, fastq)


def test_contract_and_refusals(tmp_path):
    matesdev.contract_body(engine, tmp_path)
