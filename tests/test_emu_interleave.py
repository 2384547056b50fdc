"""The bodies of test_gpu_interleave.py on the emulator (the kernel sources compiled for the host, tests/emu): k_mates_zip without a GPU.  Same
bodies, another library behind the binding; device memory lies between guard pages there and the seam allocates its output at exactly `need`
bytes, so a store behind the last piece's last byte faults at once."""
import pytest

from helpers import emu
from test_gpu_interleave import COUNTS, boundaries_body, contract_body, empties_body, phases_body, random_body


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.mark.parametrize("n", COUNTS)
def test_random_pieces_equal_the_join(n):
    random_body(n)


def test_all_pieces_empty_and_one_stream_empty():
    empties_body()


def test_every_source_and_destination_phase():
    phases_body()


def test_pieces_at_the_team_and_group_boundaries():
    boundaries_body()


def test_sizes_capacity_guard_bytes_and_refusals():
    contract_body()
