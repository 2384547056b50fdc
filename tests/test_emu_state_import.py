"""The bodies of test_gpu_state_import.py on the emulator (the kernel sources compiled for the host, tests/emu): k_import_state and the
resumed runs without a GPU.  Same bodies, another library behind the binding; device memory lies between guard pages there, so a field
read past the end of the record buffer faults at once.

By default the split runs use the pigeonhole seed kernel only; SMR_EMU_FULL=1 adds the DFS kernel, as the golden tests do."""
import os

import pytest

from helpers import emu
from test_gpu_state_import import (SPLITS, split_body, round_trip_body, resume_finished_body, boundaries_body, refusals_body, after_idcov_body)

FULL = os.environ.get("SMR_EMU_FULL", "0") == "1"
_MODES = [0, 1] if FULL else [0]


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.mark.parametrize("mode", _MODES, ids=lambda m: "dfs" if m else "pg")
@pytest.mark.parametrize("case,k", SPLITS, ids=["%s@%d" % ck for ck in SPLITS])
def test_a_split_run_equals_the_unsplit_run_and_the_reference_records(case, k, mode):
    split_body(case, k, mode)


def test_import_then_fetch_is_the_identity():
    round_trip_body()


@pytest.mark.parametrize("mode", _MODES, ids=lambda m: "dfs" if m else "pg")
def test_a_finished_run_resumes_on_a_further_db_like_the_oracle(mode):
    resume_finished_body(mode)


def test_the_parser_at_its_boundaries():
    boundaries_body()


def test_refusals_leave_a_fresh_batch_and_a_usable_context():
    refusals_body()


def test_import_after_the_id_coverage_pass_is_a_state_error():
    after_idcov_body()
