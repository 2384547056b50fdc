"""The DEFLATE kernels (csrc/smr_gzip.hpp) through smr_gzip_batch, smr_fastx_split_gz and smr_fastx_denovo_gz.  The bodies are those of
helpers/gzipdev.py; every yardstick is Python's gzip / zlib or the host model of the FASTX split, never the code under test.
test_emu_gzip.py runs the same bodies on the kernel emulator."""
import pytest

from helpers import gzipdev as g

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(g.INPUT_NAMES))
def test_round_trip_framing_and_bound(name):
    g.round_trip_body([name])


def test_eight_streams_in_one_call():
    g.eight_streams_body()


def test_repeats_at_the_farthest_distance_and_one_beyond():
    if g.chunk() < 32769 + 1000:
        pytest.skip("a chunk of %d bytes holds no repeat at distance 32 768" % g.chunk())
    g.far_body()


def test_fibonacci_frequencies_inflate():
    g.literal_limit_body()


def test_a_code_length_alphabet_that_asks_for_more_than_7_bits():
    g.code_length_limit_body()


def test_incompressible_bytes_stay_within_the_bound():
    g.incompressible_body()


def test_random_letters_take_less_than_half():
    g.fasta_body()


def test_amplicon_reads_beat_huffman_coding_alone():
    g.amplicon_body(1 << 20)


def test_determinism():
    g.determinism_body()


def test_the_batch_calls_contract():
    g.batch_contract_body()


@pytest.mark.parametrize("n_rec", [1, 64, 65, 1025])
def test_split_gz_inflates_to_the_siblings_streams(n_rec, tmp_path):
    g.split_gz_body(n_rec, tmp_path)


def test_split_gz_over_two_batches(tmp_path):
    g.split_gz_two_batches_body(tmp_path)


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
def test_denovo_gz_inflates_to_the_siblings_streams(fastq, tmp_path):
    g.denovo_gz_body(tmp_path, fastq)


def test_guards(tmp_path):
    g.guards_gz_body(tmp_path)
