"""GPU (`-m gpu`): the two Smith-Waterman kernels of production at kernel level -- k_sw16<13 | 19 | 26 | 32> (smr_walk.hpp: sixteen tasks per wave
over the packed read records, launched through smr_sw16_batch as the candidate walk launches it) and the long-read strips sw_wave_long_r<8 ... 24>
(smr_chain.hpp, through smr_ssw_batch mode 5) -- against the answers of the reference's own ssw.c (tests/golden/sw16_pairs.json,
ssw_pairs_long.json.gz) and against the plain DP of helpers/swdp.py on task lists drawn on the spot.  All comparisons are of integers and exact.
tests/test_emu_sw16.py runs the same bodies on the kernel emulator."""
import pytest

import sortmerna_amd as smr
from helpers import sw16

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = smr.Engine(0)      # raises without a GPU / without the HIP library: no CPU fallback
    yield e
    e.close()


@pytest.mark.parametrize("rows", sw16.ROWS)
def test_k_sw16_equals_the_reference_ssw_c(engine, rows):
    """every stored pair whose span k_sw16<rows> takes, on both strands, in list A (five numbers, through the begin-cell pass) and list B (score)"""
    assert sw16.check_fixture(engine, rows) == sw16.fixture_size(rows)
    if rows == 32:
        assert sw16.fixture_size(32) == 4 * sum(len(c["reads"]) for c in sw16.load())      # no stored pair is outside the widest instantiation
    assert sw16.check_fixture(engine, rows, blocks=2) == sw16.fixture_size(rows)           # ... and with two blocks: many passes per block


def test_zero_score_pairs_and_the_other_stored_pairs_through_every_kernel_of_smr_ssw_batch(engine):
    """regression: for a pair without a positive cell smr_ssw_batch reported the kernels' placeholder read_end1 = m - 1, ssw.c says 0 (sw16_pairs.json
    holds 14 such pairs; no record ever depended on it, a score of 0 is never accepted)"""
    assert sw16.check_fixture_through_ssw_batch(engine) == 5 * sum(len(c["reads"]) for c in sw16.load())


def test_long_read_strips_equal_the_reference_ssw_c(engine):
    """smr_ssw_batch mode 5 (sw_wave_any_t, forward and reverse pass) on every stored long pair; every strip height 8 ... 24 selected by at least three lengths"""
    n, heights = sw16.check_long(engine)
    assert n == sum(len(c["reads"]) for c in sw16.load_long())
    assert sorted(heights) == list(range(8, 25, 2)) and min(heights.values()) >= 3, heights


@pytest.mark.parametrize("rows", sw16.ROWS)
def test_k_sw16_equals_the_plain_dp_on_drawn_task_lists(engine, rows):
    sc = sw16.SCHEMES[sw16.ROWS.index(rows) % 2]
    for seed in (1, 2, 3):
        assert sw16.check_mixed_waves(engine, rows, sw16.SCHEMES[seed % 2], seed) == sw16.N_MIXED
    assert sw16.check_every_quad_position(engine, rows, sc) == sw16.N_POSITIONS
    assert sw16.check_hasn_on_windows_without_n(engine, rows, sc) == sw16.N_HASN
    assert sw16.check_list_sizes_and_grids(engine, rows, sc) == sw16.N_LISTS


def test_k_sw16_tasks_outside_the_range_are_refused(engine):
    assert sw16.check_refusals(engine) == 9
