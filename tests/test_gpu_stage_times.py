"""smr_rows_times, smr_pairwise_times, smr_otu_times, smr_fastx_split_times, smr_gzip_times: what a sizes-only call, a full call, a call on an
empty batch and a call of another family leave in them (helpers/stage_times.py), on the device.  One context, every call made once.

test_emu_stage_times.py runs the same body on the kernel emulator."""
import pytest

from helpers import stage_times
from test_gpu_state_import import case_setup, engine

pytestmark = pytest.mark.gpu


def test_the_writers_keep_the_timing_contract():
    stage_times.body(engine, case_setup)
