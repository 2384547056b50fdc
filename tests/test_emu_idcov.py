"""The %id / %coverage pass (csrc/smr_idcov.hpp: k_idcov_collect, k_idcov_few, k_idcov_many) compiled for the host against the wave64
emulator of tests/emu: align -> traceback -> idcov_part must leave the reference's records AFTER denovo_stats (tests/golden/otu/, written
by the unmodified reference under -otu_map -de_novo_otu) byte for byte and its four Readstats totals.  The same bodies run on the GPU
in test_gpu_idcov.py."""
import pytest

import sortmerna_amd as smr
from helpers import emu, otu


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.fixture(scope="module")
def engine(emulator):
    e = smr.Engine(0)
    yield e
    e.close()


@pytest.mark.parametrize("case", ["syn", "real"])
def test_records_after_the_pass_equal_the_reference_after_denovo_stats(engine, case, tmp_path):
    otu.body_records_and_totals(engine, case, tmp_path)


def test_without_the_pass_the_four_counters_are_zero(engine, tmp_path):
    otu.body_without_the_pass_the_counters_are_zero(engine, "syn", tmp_path)


def test_pass_before_traceback_is_a_state_error_and_thresholds_are_checked(engine, tmp_path):
    otu.body_pass_before_traceback_is_a_state_error(engine, "syn", tmp_path)


def test_handmade_triples_through_the_seam(engine):
    otu.body_handmade_triples(engine)
