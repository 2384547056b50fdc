"""k_sw16h<R> (packed f16, three-operand maxima) on the wave64 kernel emulator (tests/emu), whose f16 operations work on bit patterns through a
correctly rounded conversion (tests/emu/shim/smr_h16_ops.hpp): a value outside the integers f16 holds would come back rounded and differ from
ssw.c's stored answers and the plain DP.  Every body runs with the switch on and again with it off, so k_sw16<R> stays covered; the launch
counter of smr_sw16_f16 proves which kernel ran (helpers/sw16_f16.py).  tests/test_gpu_sw16_f16.py runs the same bodies on the GPU."""
import pytest

import sortmerna_amd as smr
from helpers import emu, sw16, sw16_f16 as h16, walk_prefix as wp


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.fixture(scope="module")
def engine(emulator):
    e = smr.Engine(0)
    yield e
    e.close()


def test_the_context_starts_with_the_f16_kernel_on_and_the_counter_at_zero(emulator):
    e = smr.Engine(0)                                       # (smr_create ran both kernels over its self-check cases: they agreed, and the counter does not show them)
    try:
        assert e.sw16_f16() == (1, 0)
        assert e.sw16_f16(0) == (0, 0) and e.sw16_f16(7) == (0, 0) and e.sw16_f16(1) == (1, 0)
    finally:
        e.close()


def test_the_switch_in_the_environment_turns_the_f16_kernel_off(emulator, monkeypatch):
    monkeypatch.setenv("SMR_SW16_F16", "0")
    e = smr.Engine(0)
    try:
        assert e.sw16_f16() == (0, 0)
    finally:
        e.close()


@pytest.mark.parametrize("on", (1, 0))
@pytest.mark.parametrize("rows", (13, 32))
def test_stored_pairs_equal_the_reference_ssw_c(engine, rows, on):
    assert h16.check_fixture(engine, rows, on) == sw16.fixture_size(rows)


@pytest.mark.parametrize("on", (1, 0))
@pytest.mark.parametrize("scheme", (0, 1))
def test_drawn_task_lists_equal_the_plain_dp(engine, scheme, on):
    assert h16.check_drawn(engine, 19, h16.SCHEMES[scheme], on) == sw16.N_MIXED + sw16.N_POSITIONS + sw16.N_HASN + sw16.N_LISTS


@pytest.mark.parametrize("on", (1, 0))
@pytest.mark.parametrize("scheme", (0, 1))
def test_prefix_intervals_equal_the_plain_dp(engine, scheme, on):
    assert h16.check_prefix(engine, 19, h16.SCHEMES[scheme], on) > 0


@pytest.mark.parametrize("on", (1, 0))
@pytest.mark.parametrize("scheme", (0, 1))
def test_top_of_the_range_one_row_short_windows_and_begin_cells(engine, scheme, on):
    assert h16.check_edges(engine, h16.SCHEMES[scheme], on) == h16.N_EDGES


def test_schemes_outside_the_predicate_take_the_integer_kernel(engine):
    assert h16.check_outside(engine) == 3 * 8


def test_the_scheme_with_gap_ext_below_half_the_mismatch_is_refused_for_every_kernel(engine):
    tl = sw16.TaskList(1)
    tl.add_problem(b"\x00\x01\x02\x03", b"\x00\x01\x02\x03", [0, 0, 0, 0, 0], 0)
    with pytest.raises(smr.SmrError, match="supported range"):
        tl.run(engine, 19, h16.REFUSED)


@pytest.mark.parametrize("on", (0, 1))
def test_records_of_a_family_workload_equal_the_oracle_with_the_switch_off_and_on(emulator, tmp_path_factory, monkeypatch, on):
    monkeypatch.setenv("SMR_SW16_F16", str(on))
    monkeypatch.setenv("SMR_SW_SELFCHECK", "0")
    w = wp.workload(tmp_path_factory.mktemp("sw16_f16_%d" % on), 300)
    exp, ctr = w.oracle_records()
    e = smr.Engine(0)
    try:
        got, c = w.gpu_records(e)
        mode, n_h = e.sw16_f16()
        walk, begins = e.sw16_launches()
        assert mode == on and sum(walk.values()) > 0 and sum(begins.values()) > 0
        assert n_h == (sum(walk.values()) + sum(begins.values()) if on else 0)
        assert got == exp, "%d records differ" % sum(1 for a, b in zip(got, exp) if a != b)
        assert c["num_aligned"] == ctr["num_aligned"]
    finally:
        e.close()
