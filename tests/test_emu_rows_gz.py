"""The bodies of test_gpu_rows_gz.py on the emulator (the kernel sources compiled for the host, tests/emu): the rows and pairwise kernels, the
line cuts and the DEFLATE kernels behind them without a GPU.  Same bodies, another library behind the binding."""
import pytest

from helpers import emu
from helpers import rowsgzdev as g


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("n", [1, 65, 1025])
def test_rows_gz_inflates_to_the_rows_of_the_sibling(n, fastq):
    g.crafted_body(n, fastq)


@pytest.mark.parametrize("n", [1, 65, 1025])
def test_pairwise_gz_inflates_to_the_text_of_the_sibling(n):
    g.crafted_body(n, n != 65, pairwise=True)


def test_two_db_golden_workload_members_hold_whole_rows():
    g.golden_body("two_db_default")


def test_contract_and_refusals():
    g.refusals_body()
