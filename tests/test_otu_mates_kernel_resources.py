"""CPU: what the compiler made of the two kernels of csrc/smr_otu_mates.hpp, read from the gfx950 code object inside libsmr_hip.so (no GPU
needed), in the manner of test_otu_kernel_resources.py.  Neither may use scratch or spill a vector register.  Their LDS is their plain
siblings': k_otu_mates_pairs none, like k_otu_pairs; k_otu_mates_write four windows of ROWS_WINDOW bytes and 16 dwords each, like k_otu_write.
Their vector registers stay within the bound that test holds the siblings to: 64, the 8 waves per SIMD of kernels that wait for memory
(the build this was written against gives 19 and 61).  Resource numbers only."""
from test_kernel_resources import _find, _kernel_metadata
from test_otu_kernel_resources import DECLARED

# name: the plain sibling whose LDS and register bound it shares
SIBLING = {"k_otu_mates_pairs": "k_otu_pairs", "k_otu_mates_write": "k_otu_write"}


def test_the_mates_kernels_use_no_scratch_and_stay_within_their_siblings_bounds():
    md = _kernel_metadata()
    for name, sibling in SIBLING.items():
        lds, vgpr_bound, _ = DECLARED[sibling]
        found = _find(md, name)
        assert len(found) == 1, name
        k = found[0]
        assert k["scratch"] == 0 and k["spill"] == 0, (name, k)
        assert k["lds"] <= lds, (name, k)
        assert k["vgpr"] <= vgpr_bound, (name, k)
        plain = _find(md, sibling)
        assert len(plain) == 1 and k["lds"] <= plain[0]["lds"], (name, k, plain)      # (the siblings are still found alone: no name is a prefix of the other's)
