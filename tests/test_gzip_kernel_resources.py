"""CPU: what the compiler made of the DEFLATE kernels of csrc/smr_gzip.hpp, read from the gfx950 code object inside libsmr_hip.so (no GPU
needed), in the manner of test_otu_kernel_resources.py.  None of them may use scratch or spill a vector register (the canonical-code counters
of k_gz_codes, indexed by a code length, live in LDS for that reason); registers are pinned at what the build gives and bounded at 64 (8 waves
per SIMD).  LDS: k_gz_match declares the hash table of 2^14 positions, the 320 symbol counters, the CRC table with its eight operators, two
rows of 256 next-pointers, 256 marks and ten words of sums and carries -- under half of a CU's 160 KiB, so that two workgroups share one;
k_gz_codes the arrays of one Huffman build over 286 symbols; k_gz_encode the two code tables and the bit window of one tile of 256 tokens."""
from test_kernel_resources import _find, _kernel_metadata

CU_LDS = 160 * 1024
MATCH_LDS = (1 << 14) * 4 + 320 * 4 + (256 + 8 * 32) * 4 + 2 * 256 * 2 + 256 + (4 + 2 + 4) * 4
ENCODE_LDS = (288 + 32) * 4 + (2 * 256 + 4) * 4 + 4 * 4
# name: (LDS bytes, VGPR bound, VGPRs of the build this was written against)
DECLARED = {"k_gz_match": (MATCH_LDS, 64, 40), "k_gz_codes": (7268, 64, 34), "k_gz_encode": (ENCODE_LDS, 64, 58), "k_gz_compact": (0, 64, 8)}


def test_the_gzip_kernels_use_no_scratch_and_only_the_lds_they_declare():
    md = _kernel_metadata()
    for name, (lds, vgpr, built) in DECLARED.items():
        found = _find(md, name)
        assert len(found) == 1, name
        for k in found:
            assert k["scratch"] == 0 and k["spill"] == 0, (name, k)
            assert k["vgpr"] == built, (name, k)                # pinned at what the build gives (DESIGN.md quotes these)
            assert built <= vgpr, name
            assert k["lds"] == lds, (name, k)


def test_two_workgroups_of_the_matching_kernel_share_a_cu():
    k = _find(_kernel_metadata(), "k_gz_match")[0]
    assert 2 * k["lds"] <= CU_LDS, k
