"""smr_gzip_lines_batch: the DEFLATE kernels over chunks that k_gz_cut_lines (csrc/smr_gzip.hpp) cuts at line ends -- nominal cuts every 48 KiB
of a stream, each moved back to behind the last newline of the 16 KiB in front of it, a hard cut where that window holds none.  The bodies
are those of helpers/rowsgzdev.py: zlib inflates every output member by member, and a model of the rule says where every member must end.
For every text: the inflation, the member count and sizes, the cuts, the bound, sizes-only against writing, one byte short, two calls.
test_emu_gzip_lines.py runs the same bodies on the kernel emulator."""
import pytest

from helpers import rowsgzdev as g

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", g.TEXT_NAMES)
def test_members_end_where_the_rule_says(name):
    g.text_body(name)


def test_eight_streams_with_a_one_byte_and_an_empty_stream():
    g.eight_streams_body()


def test_arguments_and_the_bound():
    g.arguments_body()
