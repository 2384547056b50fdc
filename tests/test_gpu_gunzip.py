"""The DEFLATE decoder kernels (csrc/smr_gunzip.hpp) through smr_gunzip_batch and smr_reads_upload_fastx* under SMR_FASTX_INFLATE.  The bodies are
those of helpers/gunzipdev.py; every yardstick is Python's zlib / gzip, never the code under test.  test_emu_gunzip.py runs the same bodies on
the kernel emulator."""
import pytest

from helpers import gunzipdev as g

pytestmark = pytest.mark.gpu


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


def test_a_large_file_without_candidates_is_the_hosts():
    g.sparse_body()


def test_upload_into_another_batch(tmp_path):
    g.upload_other_batch_body(tmp_path)


def test_upload_refusals_are_those_of_the_call_without_the_flag(tmp_path):
    g.upload_refusals_body(tmp_path)


def test_the_amplicon_fixture():
    g.amplicon_body(0)
