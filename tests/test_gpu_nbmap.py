"""GPU: the per-key bitmap of the half-seed searches that can accept a string (csrc/smr_nbmap.hpp, SMR_SEED_NBMAP) -- its builder against a host
computation, the searches with the filter forced against the unfiltered ones and the oracle, the auto policy, and the kernel's byte count.
The bodies are in helpers/nbmap_cases.py; tests/test_emu_nbmap.py runs what fits the emulator's memory on the same kernel source."""
import numpy as np
import pytest

import sortmerna_amd as smr
from helpers import nbmap_cases as nc
from helpers.workload import Workload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wl(tmp_path_factory):
    return Workload(str(tmp_path_factory.mktemp("wl")))


# L = 18 at every projection the measurements compare, and under a budget that leaves seven chars; L = 10 (pw = 5: the whole map compared, every
# pattern against every string; a budget that raises the drop); L = 14 and 16 (other pw and h).  The index builder makes parts of L = 8..18, so a
# part of L = 20 -- whose exact set has slabs of 128 KB, which the 32 KB rule answers by dropping a char -- cannot be made here.
@pytest.mark.parametrize("lnwin,db_nt,drop,host_layout,budget", [
    (18, 400_000, 0, False, None), (18, 400_000, 1, True, None), (18, 400_000, 2, False, None), (18, 400_000, 0, True, 2 * nc.GIB),
    (10, 60_000, 0, False, None), (10, 60_000, 1, True, None), (10, 60_000, 0, True, 100_000),
    (16, 400_000, 0, False, None), (14, 200_000, 1, True, None)],
    ids=["L18-s0-dev", "L18-s1-host", "L18-s2-dev", "L18-budget2G-host", "L10-s0-dev", "L10-s1-host", "L10-budget-host", "L16-s0-dev", "L14-s1-host"])
def test_builder_equals_a_host_computation(tmp_path, monkeypatch, lnwin, db_nt, drop, host_layout, budget):
    nc.builder_body(tmp_path, monkeypatch, lnwin, db_nt, drop, host_layout, budget)


@pytest.mark.parametrize("drop", [0, 1, 2])
def test_seed_scan_with_the_filter_forced_equals_the_unfiltered_scan(wl, monkeypatch, drop):
    assert nc.scan_parity_body(wl, monkeypatch, drop)["drop"] == drop


@pytest.mark.parametrize("drop", [0, 1, 2])
@pytest.mark.parametrize("env", [None, {"SMR_SEED_SHARED": "2", "SMR_SEED_DEDUP": "2", "SMR_SEG_INLINE": "0"}], ids=["default", "shared-dedup-seg_inline_off"])
def test_records_with_the_filter_forced_equal_the_oracle(wl, monkeypatch, drop, env):
    nc.records_parity_body(wl, monkeypatch, drop, env=env)


def test_multi_part_index_with_two_references_and_the_filter_forced(tmp_path, monkeypatch):
    nc.two_refs_body(tmp_path, monkeypatch, 1)


def test_auto_policy(wl, tmp_path, monkeypatch):
    nc.policy_body(wl, tmp_path, monkeypatch)


@pytest.fixture(scope="module")
def wl_small(tmp_path_factory):
    """(the host recount walks every search in Python: a third of the reads keeps it to seconds)"""
    return Workload(str(tmp_path_factory.mktemp("wls")), n_reads=1200)


@pytest.mark.parametrize("strand,pass_,drop", [(0, 0, 0), (1, 2, 0), (0, 0, 2), (1, 2, 1)])
def test_pigeonhole_search_bytes_with_the_filter_equal_a_host_recount(wl_small, monkeypatch, strand, pass_, drop):
    nc.bytes_body(wl_small, monkeypatch, strand, pass_, drop)
