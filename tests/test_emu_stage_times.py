"""The body of test_gpu_stage_times.py on the emulator (the engine's host code compiled for the host, tests/emu): when the device report
writers start, fill and leave alone the times of their families.  Same body, another library behind the binding."""
import pytest

from helpers import emu, stage_times
from test_gpu_state_import import case_setup, engine


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


def test_the_writers_keep_the_timing_contract():
    stage_times.body(engine, case_setup)
