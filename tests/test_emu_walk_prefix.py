"""A slice of tests/test_gpu_walk_prefix.py on the wave64 kernel emulator (tests/emu): 700 reads of the same family workload; every mode and
option set with SMR_WALK_K = 4, and the two modes that leave prefix tasks under best 1 with SMR_WALK_K = 15 and 1 (helpers/walk_prefix.py)."""
import pytest

from helpers import emu, walk_prefix as wp

CASES = [(mode, 4, opt) for mode in wp.MODES for opt in wp.OPTIONS] + [(mode, k, "best1") for mode in ("cols4", "cols40pct") for k in (15, 1)]


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.fixture(scope="module")
def family(emulator, tmp_path_factory):
    w = wp.workload(tmp_path_factory.mktemp("walk_prefix"), 700)
    return w, wp.Oracle(w)


@pytest.mark.parametrize("mode,k,opt", CASES)
def test_records_equal_the_oracle_under_every_prefix_mode(family, monkeypatch, mode, k, opt):
    wp.run_case(family[0], family[1], monkeypatch, mode, k, opt)


def test_an_undecided_interval_met_in_the_closing_round_is_scored_inside_k_walk(family, monkeypatch):
    st = wp.run_case(family[0], family[1], monkeypatch, "cols4", 4, "best1", rounds=2)
    assert st["redone"] > 0, st


def test_a_context_stops_leaving_prefix_tasks_after_a_part_they_did_not_decide(family, monkeypatch):
    wp.check_back_off(family[0], family[1], monkeypatch)
