"""smr_otu_part_mates: the members of otu_map.txt of mates that were read from two files (read i of batch 0 and read i of batch 1), classified
and sized per batch by the kernels of smr_otu_part, merged by k_otu_mates_pairs into the order of smr_report_add_pair, then sorted and written
(csrc/smr_otu_mates.hpp, csrc/smr_engine_otu.hpp).

The yardstick of every test is the host writer fed pair by pair (Report.add_pair), never the code under test; for the reference's paired
fixture also the otu_map.txt the reference wrote.  Bodies in helpers/otu_mates.py:

1. crafted state in batches 0 and 1: 1, 63, 64, 65, 255, 256, 257, 1025 pairs, FASTA and FASTQ -- members in batch A only, in B only, in both,
   mate 2 passing next to a mate 1 without a counter, a counter without a passing slot of the key, several slots on different references;
   every member in one group (4100 of them at 1025 pairs); all members in one batch; ids of A and B of different length and content;
2. an id of more than the 4 KB window in batch B next to short ids of A;
3. the reference's paired fixture (tests/golden/paired, tests/golden/otu) in two batches;
4. the contract and every refusal of include/smr_hip.h, in their precedence.

test_emu_otu_mates.py runs the same bodies on the kernel emulator."""
import pytest

from helpers import otu_device as od
from helpers import otu_mates as om
from test_gpu_state_import import engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("n", om.COUNTS)
def test_crafted_mates_give_the_host_writers_map(n, fastq, tmp_path):
    om.crafted_body(engine, n, "mixed", fastq, tmp_path)


@pytest.mark.parametrize("n,fastq", [(1, True), (65, False), (1025, True)])
def test_one_reference_takes_every_member(n, fastq, tmp_path):
    om.crafted_body(engine, n, "one", fastq, tmp_path)


@pytest.mark.parametrize("shape,n,fastq", [("a only", 65, True), ("b only", 65, False), ("a only", 257, False), ("b only", 257, True)])
def test_members_in_one_batch_only(shape, n, fastq, tmp_path):
    om.crafted_body(engine, n, shape, fastq, tmp_path)


def test_a_long_id_in_batch_b_next_to_short_ids_in_a(tmp_path):
    om.crafted_body(engine, 70, "one", True, tmp_path, long_at=35)
    om.crafted_body(engine, 67, "one", False, tmp_path / "fasta", long_at=3)


@pytest.mark.parametrize("case", od.PAIRED)
def test_the_paired_fixture_in_two_batches(case, tmp_path):
    assert om.paired_body(engine, case, tmp_path) == (case in ("paired_loose", "paired_loose_in"))


def test_contract_and_refusals(tmp_path):
    om.contract_body(engine, tmp_path)
