"""The bodies of tests/test_gpu_sw16.py on the wave64 kernel emulator (tests/emu): k_sw16<13 | 19 | 26 | 32> through smr_sw16_batch and the
long-read strips through smr_ssw_batch mode 5 against ssw.c's stored answers and the plain DP.  The emulator runs these kernels at a few million
cells per second, so the default run already holds every stored k_sw16 pair for every instantiation (both strands, both lists, both directions)
and the drawn task lists; only the long pairs are a slice by default (the cheapest pair of every strip height), all of them with SMR_EMU_FULL=1."""
import os

import pytest

import sortmerna_amd as smr
from helpers import emu, sw16

FULL = os.environ.get("SMR_EMU_FULL", "0") == "1"


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.fixture(scope="module")
def engine(emulator):
    e = smr.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("rows", sw16.ROWS)
def test_k_sw16_equals_the_reference_ssw_c(engine, rows):
    assert sw16.check_fixture(engine, rows) == sw16.fixture_size(rows)
    if rows == 32:
        assert sw16.fixture_size(32) == 4 * sum(len(c["reads"]) for c in sw16.load())
    if FULL:
        assert sw16.check_fixture(engine, rows, blocks=2) == sw16.fixture_size(rows)


def test_zero_score_pairs_and_the_other_stored_pairs_through_every_kernel_of_smr_ssw_batch(engine):
    """regression: for a pair without a positive cell smr_ssw_batch reported the kernels' placeholder read_end1 = m - 1, ssw.c says 0 (sw16_pairs.json
    holds 14 such pairs; no record ever depended on it, a score of 0 is never accepted)"""
    assert sw16.check_fixture_through_ssw_batch(engine) == 5 * sum(len(c["reads"]) for c in sw16.load())


def test_long_read_strips_equal_the_reference_ssw_c(engine):
    n, heights = sw16.check_long(engine, None if FULL else sw16.cheapest_long_pair_per_height(engine))
    assert sorted(heights) == list(range(8, 25, 2)), heights
    if FULL:
        assert n == sum(len(c["reads"]) for c in sw16.load_long()) and min(heights.values()) >= 3, heights
    else:
        assert n == 9


@pytest.mark.parametrize("rows", sw16.ROWS)
def test_k_sw16_equals_the_plain_dp_on_drawn_task_lists(engine, rows):
    sc = sw16.SCHEMES[sw16.ROWS.index(rows) % 2]
    for seed in (1, 2, 3) if FULL else (1,):
        assert sw16.check_mixed_waves(engine, rows, sw16.SCHEMES[seed % 2], seed) == sw16.N_MIXED
    assert sw16.check_every_quad_position(engine, rows, sc) == sw16.N_POSITIONS
    assert sw16.check_hasn_on_windows_without_n(engine, rows, sc) == sw16.N_HASN
    assert sw16.check_list_sizes_and_grids(engine, rows, sc) == sw16.N_LISTS


def test_k_sw16_tasks_outside_the_range_are_refused(engine):
    assert sw16.check_refusals(engine) == 9
