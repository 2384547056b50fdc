"""The bodies of test_gpu_gzip_lines.py on the emulator (the kernel sources compiled for the host, tests/emu): k_gz_cut_lines and the DEFLATE
kernels behind it without a GPU.  Same bodies, another library behind the binding; device memory lies between guard pages there, so a load
in front of a stream's first window or behind its last byte faults at once."""
import pytest

from helpers import emu
from helpers import rowsgzdev as g


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.mark.parametrize("name", g.TEXT_NAMES)
def test_members_end_where_the_rule_says(name):
    g.text_body(name)


def test_eight_streams_with_a_one_byte_and_an_empty_stream():
    g.eight_streams_body()


def test_arguments_and_the_bound():
    g.arguments_body()
