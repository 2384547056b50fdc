"""The bodies of test_gpu_gunzip.py on the emulator (the kernel sources compiled for the host, tests/emu): the DEFLATE decoder kernels without a
GPU.  Same bodies, another library behind the binding; device memory lies between guard pages there, so a load or a store outside a buffer
faults at once.  Of the amplicon fixture the first MiB of text is used, compressed by Python."""
import pytest

from helpers import emu
from helpers import gunzipdev as g


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.mark.parametrize("name", list(g.ROUND_TRIP))
def test_round_trip_on_the_device_path_with_the_models_task_starts(name):
    g.round_trip_body(name)


def test_placeholders_across_task_boundaries():
    g.placeholders_body()


def test_five_members_and_the_device_compressors_output():
    g.members_body()


def test_a_false_candidate_is_rejected_by_the_stitch():
    g.false_candidate_body()


def test_refusals_are_zlibs():
    g.refusals_body()


def test_the_batch_calls_contract():
    g.contract_body()


@pytest.mark.parametrize("n_rec", [1, 64, 65, 1025])
@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_upload_with_inflate_equals_upload_without(fastq, n_rec, tmp_path):
    g.upload_body(fastq, n_rec, tmp_path)


def test_upload_into_another_batch(tmp_path):
    g.upload_other_batch_body(tmp_path)


def test_upload_refusals_are_those_of_the_call_without_the_flag(tmp_path):
    g.upload_refusals_body(tmp_path)


def test_the_first_mib_of_the_amplicon_fixture():
    g.amplicon_body(1 << 20)
