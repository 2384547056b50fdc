"""The bodies of test_gpu_state_export.py on the emulator (the kernel sources compiled for the host, tests/emu): the sizing kernels and
k_export_state without a GPU.  Same bodies, another library behind the binding; device memory lies between guard pages there, so a store
behind the last record's last byte faults at once."""
import pytest

from helpers import emu
from test_gpu_state_export import REAL_CASES, SMALL_N, boundaries_body, guards_body, real_run_body, after_idcov_body, split_body


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


def test_the_writer_at_its_boundaries():
    boundaries_body()


@pytest.mark.parametrize("n", SMALL_N)
def test_small_batches(n):
    boundaries_body(n)


def test_guards():
    guards_body()


@pytest.mark.parametrize("case", REAL_CASES)
def test_export_equals_fetch_and_records_at_every_step(case):
    real_run_body(case)


def test_records_after_the_id_coverage_pass_carry_the_counters(tmp_path):
    after_idcov_body(tmp_path)


@pytest.mark.parametrize("case", REAL_CASES)
def test_a_run_split_through_export_equals_the_unsplit_run(case):
    split_body(case)
