"""smr_rows_part_mates, smr_pairwise_part_mates and their _gz forms: the SAM / BLAST rows and the pairwise text of mates that were read from
two files (read i of batch 0 and read i of batch 1), written per batch by the kernels of the plain calls and interleaved on the device by
k_mates_zip (csrc/smr_mates.hpp, csrc/smr_engine_mates.hpp).

The yardstick of every test is the host writer fed pair by pair (Report.add_pair, pinned to the reference's files by test_reports_cpu.py),
never the code under test; for the _gz forms it is zlib and gzip_lines_batch of the plain bytes.  Bodies in helpers/matesdev.py:

1. crafted state (helpers/rows.py: craft, two seeds) in batches 0 and 1: 1, 63, 64, 65, 255, 256, 257, 1025 pairs, FASTA and FASTQ; SAM only, BLAST
   with all optional columns, both; the pairwise text; pairs with rows in one batch only, in both, in neither; rows of both batches at all
   four byte phases; a 5 kb read in batch 1 next to short rows in batch 0;
2. the reference's paired fixture (tests/golden/paired) aligned and traced back in two batches;
3. the _gz forms;
4. the contract and every refusal of include/smr_hip.h, in their precedence.

test_emu_rows_mates.py runs the same bodies on the kernel emulator."""
import pytest

from helpers import matesdev
from test_gpu_state_import import engine

pytestmark = pytest.mark.gpu


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
