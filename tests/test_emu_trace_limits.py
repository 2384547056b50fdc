"""The bodies of tests/test_gpu_trace_limits.py on the wave64 kernel emulator (tests/emu): k_trace_band<8 | 16> and k_trace_wide through smr_cigar_batch
against the CIGARs ssw.c's banded_sw returned for pairs constructed on the kernels' limits (tests/golden/trace_limits.json.gz).  The default run holds
every stored pair, every rung assertion up to band 255, the mixed batches and both switch variants; it leaves out only (all of it with SMR_EMU_FULL=1)
  * of the gaps of 2 046 | 2 047 letters, the launch counts of the insertions (the deletions are counted; all four pairs are compared in their batch),
  * of the replication, everything beyond the smallest batch at which every kernel's grid loops on the emulator's 4 CUs (x 4 with the switch)."""
import ctypes
import os

import pytest

import sortmerna_amd as smr
from helpers import emu, tracelimits

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


def emulated_cus(lib):
    """the CU count the emulator's device reports to the engine"""
    lib.emu_multiprocessor_count.restype = ctypes.c_int
    return lib.emu_multiprocessor_count()


def test_every_stored_pair_equals_the_reference_banded_sw(engine):
    assert tracelimits.check(engine, tracelimits.CLASSES, widest_gaps=True) == len(tracelimits.pairs()) == tracelimits.N_PAIRS


def test_the_launch_count_tells_the_rung_that_finished_each_pair(engine):
    assert tracelimits.check_rungs(engine) == 152
    assert tracelimits.check_widest_rungs(engine, "ID" if FULL else "D") == (4 if FULL else 2)


@pytest.mark.parametrize("big", tracelimits.BIG_WITHOUT_NARROW + tracelimits.BIG_WITH_NARROW)
def test_short_pairs_in_one_batch_with_a_long_read(engine, big):
    assert tracelimits.check_mixed(engine, big) > 200


def test_more_tasks_than_every_grid_has_blocks(engine):
    cus = emulated_cus(ctypes.CDLL(emu.build()))
    assert cus >= 1
    assert tracelimits.check_replicated(engine, cus * (4 if FULL else 1)) > cus * 128


def test_global_rows_and_a_cigar_pool_of_16_words(emulator):
    assert tracelimits.check_switches(lambda: smr.Engine(0)) > 380
