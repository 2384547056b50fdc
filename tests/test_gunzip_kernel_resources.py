"""CPU: what the compiler made of the DEFLATE decoder kernels of csrc/smr_gunzip.hpp, read from the gfx950 code object inside libsmr_hip.so (no GPU
needed), in the manner of test_gzip_kernel_resources.py.  None of them may use scratch or spill a vector register: the code-length code of a
candidate lives in two 64-bit registers of k_gunz_find for that reason, and every array of k_gunz_decode that is indexed by a code length lives
in LDS.  Registers are pinned at what the build gives.  LDS: k_gunz_decode declares 340 bytes of code lengths, five arrays of 16 counters, the
sorted symbols of the three codes (288 + 32 + 20), the three tables (2^10 + 2^8 + 2^7 entries of 16 bits) and one status word -- 4 000 bytes,
4 of padding --, so LDS never limits the waves of a CU; k_gunz_resolve the CRC table with its eight operators and four partial sums;
k_gunz_find and k_gunz_window none.  k_gunz_window runs 1024 threads, i.e. four waves per SIMD: 128 registers at the most."""
from test_kernel_resources import _find, _kernel_metadata

DECODE_LDS = 340 + 2 * (5 * 16 + 288 + 32 + 20 + 1024 + 256 + 128) + 4 + 4
RESOLVE_LDS = (256 + 8 * 32) * 4 + 4 * 4
# name: (instances, LDS bytes, VGPR bound, VGPRs of the build this was written against)
DECLARED = {"k_gunz_find": (1, 0, 64, 50), "k_gunz_decode": (2, DECODE_LDS, 128, 80), "k_gunz_window": (1, 0, 128, 72), "k_gunz_resolve": (1, RESOLVE_LDS, 64, 38)}


def test_the_gunzip_kernels_use_no_scratch_and_only_the_lds_they_declare():
    md = _kernel_metadata()
    for name, (count, lds, vgpr, built) in DECLARED.items():
        found = _find(md, name)
        assert len(found) == count, name                        # (k_gunz_decode: the counting and the writing instance)
        for k in found:
            assert k["scratch"] == 0 and k["spill"] == 0, (name, k)
            assert k["vgpr"] == built, (name, k)                # pinned at what the build gives (DESIGN.md quotes these)
            assert built <= vgpr, name
            assert k["lds"] == lds, (name, k)
