"""smr_rows_part_gz and smr_pairwise_part_gz: the streams of smr_rows_part / smr_pairwise_part left on the device and compressed there into
gzip members that end at line ends.  The bodies are those of helpers/rowsgzdev.py; the yardsticks are the plain siblings (pinned to the host
writer by test_gpu_rows.py / test_gpu_pairwise.py), zlib, which inflates every member, and the model of the cut rule.

1. the crafted state of helpers/rows.py at 1, 65 and 1025 reads (one member, and several): SAM only, BLAST only, both, the optional columns,
   every key; plain_off, an unwanted stream without a byte, smaller than plain from 4 KiB on, every member but the last a whole number of rows;
2. the two-DB golden workload with its stored records;
3. the contract and the refusals of the plain calls, with messages that name the new calls.

test_emu_rows_gz.py runs the same bodies on the kernel emulator."""
import pytest

from helpers import rowsgzdev as g

pytestmark = pytest.mark.gpu


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
