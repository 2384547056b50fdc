"""smr_otu_part, smr_fastx_denovo and the report calls that take their streams: the members of otu_map.txt of one (index, part) classified,
compacted, sorted by reference and written by kernels (csrc/smr_otu.hpp), aligned_denovo.* routed and copied beside smr_fastx_split.

The yardstick of every test is the host writer (smr_report_add / smr_report_add_pair, pinned to the reference's own files by test_otu_cpu.py)
or the reference's files themselves (tests/golden/otu/), never the code under test.  The bodies live in helpers/otu_device.py;
test_emu_otu_device.py runs the same bodies on the kernel emulator.

1. the sort seam against numpy's stable argsort;  2. crafted state: pair counts, group shapes, ids, strands, N, long CIGARs;
3. the second rounding (`* 0.001`);  4. a map that exists and is empty;  5. the reference's files;  6. the routing table of aligned_denovo.*;
7. the contract and the refusals of include/smr_hip.h."""
import pytest

from helpers import otu_device as od
from test_gpu_state_import import case_setup, engine

pytestmark = pytest.mark.gpu

CASES = ["syn", "syn_all", "two_db", "syn_multipart", "real", "syn_denovo_only"]


def test_the_sort_is_numpys_stable_argsort():
    od.sort_body(engine)


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("shape", od.SHAPES)
@pytest.mark.parametrize("n_pairs", od.PAIR_COUNTS)
def test_crafted_state_gives_the_host_writers_map(n_pairs, shape, fastq, tmp_path):
    od.crafted_body(engine, n_pairs, shape, fastq, tmp_path, seed=n_pairs + 1)


def test_the_second_rounding_is_a_product(tmp_path):
    od.rounding_body(engine, tmp_path)


def test_a_map_that_exists_and_is_empty(tmp_path):
    od.empty_map_body(engine, tmp_path)


@pytest.mark.parametrize("case", CASES)
def test_the_device_files_equal_the_reference_files(case, tmp_path):
    od.reference_files_body(engine, case_setup, case, tmp_path)


@pytest.mark.parametrize("case", od.PAIRED)
def test_interleaved_pairs_equal_the_host_writer_and_the_reference_ids(case, tmp_path):
    od.paired_body(engine, case, tmp_path)


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_denovo_routing_equals_the_host_table(fastq, tmp_path):
    od.routing_body(engine, tmp_path, fastq)


def test_contract_and_refusals(tmp_path):
    od.contract_body(engine, tmp_path)


def test_the_report_side_refusals(tmp_path):
    od.report_side_body(tmp_path)
