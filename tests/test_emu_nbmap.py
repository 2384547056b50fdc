"""The search bitmap (csrc/smr_nbmap.hpp) on the wave64 emulator: the bodies of tests/test_gpu_nbmap.py on the same kernel source, at the sizes the
emulator's host memory allows -- the whole map of an L = 10 part, and L = 18 under a byte budget of 64 MiB, which leaves five pattern chars."""
import pytest

from helpers import emu
from helpers import nbmap_cases as nc
from helpers.workload import Workload

BUDGET = 64 << 20


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.fixture(scope="module")
def wl(tmp_path_factory, emulator):
    return Workload(str(tmp_path_factory.mktemp("wl")), db_nt=200_000, n_reads=1200)


@pytest.mark.parametrize("lnwin,db_nt,drop,host_layout,budget", [
    (10, 60_000, 0, False, None), (10, 60_000, 1, True, None), (18, 120_000, 0, False, BUDGET), (18, 120_000, 0, True, BUDGET)],
    ids=["L10-s0-dev", "L10-s1-host", "L18-budget-dev", "L18-budget-host"])
def test_builder_equals_a_host_computation(tmp_path, monkeypatch, lnwin, db_nt, drop, host_layout, budget):
    nc.builder_body(tmp_path, monkeypatch, lnwin, db_nt, drop, host_layout, budget)


def test_seed_scan_with_the_filter_forced_equals_the_unfiltered_scan(wl, monkeypatch):
    assert nc.scan_parity_body(wl, monkeypatch, 0, BUDGET)["drop"] == 4


@pytest.mark.parametrize("env", [None, {"SMR_SEED_SHARED": "2", "SMR_SEED_DEDUP": "2", "SMR_SEG_INLINE": "0"}], ids=["default", "shared-dedup-seg_inline_off"])
def test_records_with_the_filter_forced_equal_the_oracle(wl, monkeypatch, env):
    nc.records_parity_body(wl, monkeypatch, 0, BUDGET, env=env)


def test_auto_policy(wl, tmp_path, monkeypatch):
    nc.policy_body(wl, tmp_path, monkeypatch)


@pytest.mark.parametrize("strand,pass_", [(0, 0), (1, 2)])
def test_pigeonhole_search_bytes_with_the_filter_equal_a_host_recount(wl, monkeypatch, strand, pass_):
    nc.bytes_body(wl, monkeypatch, strand, pass_, 0, BUDGET)
