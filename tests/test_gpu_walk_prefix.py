"""GPU (`-m gpu`): the candidate walk with prefix tasks on a family workload (families of 40, 3 000 reads, 40 % from the DB): records, hit
count and ssw_align call count equal to the oracle's with the mode off, with prefixes of four columns, of about 40 % of a window and as long
as the window, crossed with SMR_WALK_K = 1 / 4 / 15 and four option sets; smr_walk_prefix_stats shows the path taken (helpers/walk_prefix.py).
tests/test_emu_walk_prefix.py runs a slice of it on the kernel emulator."""
import pytest

from helpers import walk_prefix as wp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def family(tmp_path_factory):
    w = wp.workload(tmp_path_factory.mktemp("walk_prefix"), 3000)
    return w, wp.Oracle(w)


@pytest.mark.parametrize("opt", list(wp.OPTIONS))
@pytest.mark.parametrize("k", wp.WALK_K)
@pytest.mark.parametrize("mode", list(wp.MODES))
def test_records_equal_the_oracle_under_every_prefix_mode(family, monkeypatch, mode, k, opt):
    wp.run_case(family[0], family[1], monkeypatch, mode, k, opt)


@pytest.mark.parametrize("mode", ["cols4", "cols40pct"])
def test_an_undecided_interval_met_in_the_closing_round_is_scored_inside_k_walk(family, monkeypatch, mode):
    st = wp.run_case(family[0], family[1], monkeypatch, mode, 4, "best1", rounds=2)
    assert st["redone"] > 0, st


def test_a_context_stops_leaving_prefix_tasks_after_a_part_they_did_not_decide(family, monkeypatch):
    wp.check_back_off(family[0], family[1], monkeypatch)
