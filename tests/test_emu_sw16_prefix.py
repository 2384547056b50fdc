"""The bodies of tests/test_gpu_sw16_prefix.py on the wave64 kernel emulator (tests/emu): the prefix tasks of k_sw16<13 | 19 | 26 | 32> through
smr_sw16_prefix_batch against the plain DP and ssw.c's stored scores.  By default every third stored pair; all of them with SMR_EMU_FULL=1."""
import os

import pytest

import sortmerna_amd as smr
from helpers import emu, sw16_prefix as pfx

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


@pytest.mark.parametrize("rows", pfx.ROWS)
def test_prefix_intervals_of_the_stored_pairs_hold_the_score_of_ssw_c(engine, rows):
    every = 1 if FULL else 3
    assert pfx.check_fixture(engine, rows, every) == pfx.fixture_size(rows, every) > 0


@pytest.mark.parametrize("rows", pfx.ROWS)
def test_prefix_intervals_equal_the_plain_dp_at_the_smallest_shapes(engine, rows):
    sc = pfx.SCHEMES[pfx.ROWS.index(rows) % 2]
    assert pfx.check_shapes(engine, rows, sc) == pfx.n_shapes(rows)
    assert pfx.check_quads_and_cols(engine, rows, sc) == pfx.N_QUADS
    assert pfx.check_list_sizes(engine, rows, sc) == pfx.N_LISTS


def test_prefix_tasks_outside_the_range_are_refused(engine):
    assert pfx.check_refusals(engine) == 5
