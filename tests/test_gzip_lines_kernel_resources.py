"""CPU: what the compiler made of k_gz_cut_lines (csrc/smr_gzip.hpp), read from the gfx950 code object inside libsmr_hip.so (no GPU needed), in
the manner of test_gzip_kernel_resources.py.  No scratch, no spilled register; registers pinned at what the build gives and bounded at 64
(8 waves per SIMD); LDS: the four words through which the waves of a workgroup exchange the last line end each of them found."""
from test_kernel_resources import _find, _kernel_metadata

CUT_LDS = 4 * 4
VGPR_BOUND, VGPR_BUILT = 64, 10


def test_the_line_cut_kernel_uses_no_scratch_and_only_the_lds_it_declares():
    found = _find(_kernel_metadata(), "k_gz_cut_lines")
    assert len(found) == 1, found
    k = found[0]
    assert k["scratch"] == 0 and k["spill"] == 0, k
    assert k["vgpr"] == VGPR_BUILT <= VGPR_BOUND, k                  # pinned at what the build gives (DESIGN.md quotes it)
    assert k["lds"] == CUT_LDS, k
