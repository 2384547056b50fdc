"""GPU: k_trace_band<8 | 16> and k_trace_wide through smr_cigar_batch against the CIGARs ssw.c's banded_sw returned for pairs constructed ON the kernels'
limits (tests/golden/trace_limits.json.gz, tests/golden/make_golden_trace_limits.py): both sides of every hand-over of the band ladder (3|4, 7|8,
31|32, 255|256, 2047|2048), strip counts 1|2|3, the outermost diagonals of a band, 19..33 CIGAR runs around the 24 that are staged, spans of 1..10
letters with windows shorter and longer than the read, random fillers across strip boundaries -- and, by the number of launches, WHICH kernel finished each of them.  tests/test_emu_trace_limits.py runs the same bodies on the emulator."""
import pytest

import sortmerna_amd as smr
from helpers import tracelimits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = smr.Engine(0)
    yield e
    e.close()


def test_every_stored_pair_equals_the_reference_banded_sw(engine):
    assert tracelimits.check(engine, tracelimits.CLASSES, widest_gaps=True) == len(tracelimits.pairs()) == tracelimits.N_PAIRS


def test_the_launch_count_tells_the_rung_that_finished_each_pair(engine):
    assert tracelimits.check_rungs(engine) == 152
    assert tracelimits.check_widest_rungs(engine) == 4


@pytest.mark.parametrize("big", tracelimits.BIG_WITHOUT_NARROW + tracelimits.BIG_WITH_NARROW)
def test_short_pairs_in_one_batch_with_a_long_read(engine, big):
    assert tracelimits.check_mixed(engine, big) > 200


def test_more_tasks_than_every_grid_has_blocks(engine):
    """an MI355X has 256 CUs: 256 x 16 blocks x 8 alignments = 32 768 tasks before k_trace_band<8> loops, 256 x 32 = 8 192 blocks of k_trace_wide"""
    assert tracelimits.check_replicated(engine, 256, at_least=40000) >= 40000


def test_global_rows_and_a_cigar_pool_of_16_words():
    assert tracelimits.check_switches(lambda: smr.Engine(0)) > 380
