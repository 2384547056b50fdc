"""The bodies of test_gpu_otu_device.py on the emulator (the kernel sources compiled for the host, tests/emu): k_otu_classify, the sort, the
writer and k_fxs_dn_measure without a GPU.  Same bodies, another library behind the binding; device memory lies between guard pages there, so
a store behind the last byte faults at once."""
import pytest

from helpers import emu
from helpers import otu_device as od
from test_gpu_state_import import case_setup, engine


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


def test_the_sort_is_numpys_stable_argsort():
    od.sort_body(engine, ns=[0, 1, 63, 64, 65, 4097])


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("shape", od.SHAPES)
@pytest.mark.parametrize("n_pairs", [0, 1, 64, 65, 1025])
def test_crafted_state_gives_the_host_writers_map(n_pairs, shape, fastq, tmp_path):
    od.crafted_body(engine, n_pairs, shape, fastq, tmp_path, seed=n_pairs + 1)


def test_the_second_rounding_is_a_product(tmp_path):
    od.rounding_body(engine, tmp_path)


def test_a_map_that_exists_and_is_empty(tmp_path):
    od.empty_map_body(engine, tmp_path)


@pytest.mark.parametrize("case", ["syn", "two_db", "syn_denovo_only"])
def test_the_device_files_equal_the_reference_files(case, tmp_path):
    od.reference_files_body(engine, case_setup, case, tmp_path)


@pytest.mark.parametrize("case", ["paired_out2_sout", "paired_loose_in"])
def test_interleaved_pairs_equal_the_host_writer_and_the_reference_ids(case, tmp_path):
    od.paired_body(engine, case, tmp_path)


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_denovo_routing_equals_the_host_table(fastq, tmp_path):
    od.routing_body(engine, tmp_path, fastq)


def test_contract_and_refusals(tmp_path):
    od.contract_body(engine, tmp_path)


def test_the_report_side_refusals(tmp_path):
    od.report_side_body(tmp_path)
