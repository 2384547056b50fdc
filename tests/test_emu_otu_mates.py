"""The bodies of test_gpu_otu_mates.py on the emulator (the kernel sources compiled for the host, tests/emu): k_otu_mates_pairs and
k_otu_mates_write without a GPU.  Same bodies, another library behind the binding; device memory lies between guard pages there, so a store
behind the last byte faults at once."""
import pytest

from helpers import emu
from helpers import otu_mates as om
from test_gpu_state_import import engine


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.mark.parametrize("n,fastq", [(1, False), (64, True), (65, False), (257, True), (1025, False)])
def test_crafted_mates_give_the_host_writers_map(n, fastq, tmp_path):
    om.crafted_body(engine, n, "mixed", fastq, tmp_path)


@pytest.mark.parametrize("n,fastq", [(1, True), (1025, True)])
def test_one_reference_takes_every_member(n, fastq, tmp_path):
    om.crafted_body(engine, n, "one", fastq, tmp_path)


@pytest.mark.parametrize("shape,n,fastq", [("a only", 65, True), ("b only", 65, False)])
def test_members_in_one_batch_only(shape, n, fastq, tmp_path):
    om.crafted_body(engine, n, shape, fastq, tmp_path)


def test_a_long_id_in_batch_b_next_to_short_ids_in_a(tmp_path):
    om.crafted_body(engine, 70, "one", True, tmp_path, long_at=35)
    om.crafted_body(engine, 67, "one", False, tmp_path / "fasta", long_at=3)


@pytest.mark.parametrize("case", ["paired_out2_sout", "paired_loose_in"])
def test_the_paired_fixture_in_two_batches(case, tmp_path):
    assert om.paired_body(engine, case, tmp_path) == (case == "paired_loose_in")


def test_contract_and_refusals(tmp_path):
    om.contract_body(engine, tmp_path)
