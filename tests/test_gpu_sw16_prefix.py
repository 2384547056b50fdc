"""GPU (`-m gpu`): the prefix tasks of k_sw16<13 | 19 | 26 | 32> (smr_walk.hpp, SW16_PREFIX) at kernel level, through smr_sw16_prefix_batch: lo is the
plain DP's maximum over the first cols columns, hi the stated bound on the DP's row maxima, and the score of the whole window (ssw.c's for the
stored pairs of tests/golden/sw16_pairs.json, the plain DP's for drawn ones) lies between them.  All comparisons are of integers and exact.
tests/test_emu_sw16_prefix.py runs the same bodies on the kernel emulator."""
import pytest

import sortmerna_amd as smr
from helpers import sw16_prefix as pfx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = smr.Engine(0)      # raises without a GPU / without the HIP library: no CPU fallback
    yield e
    e.close()


@pytest.mark.parametrize("rows", pfx.ROWS)
def test_prefix_intervals_of_the_stored_pairs_hold_the_score_of_ssw_c(engine, rows):
    assert pfx.check_fixture(engine, rows) == pfx.fixture_size(rows) > 0


@pytest.mark.parametrize("rows", pfx.ROWS)
def test_prefix_intervals_equal_the_plain_dp_at_the_smallest_shapes(engine, rows):
    sc = pfx.SCHEMES[pfx.ROWS.index(rows) % 2]
    assert pfx.check_shapes(engine, rows, sc) == pfx.n_shapes(rows)
    assert pfx.check_quads_and_cols(engine, rows, sc) == pfx.N_QUADS
    assert pfx.check_list_sizes(engine, rows, sc) == pfx.N_LISTS


def test_prefix_tasks_outside_the_range_are_refused(engine):
    assert pfx.check_refusals(engine) == 5
