"""CPU: what the compiler made of the kernels of csrc/smr_pairwise.hpp, read from the gfx950 code object inside libsmr_hip.so (no GPU needed), in
the manner of test_rows_kernel_resources.py.  Neither may use scratch or spill a vector register.  Registers, from what the build gives:
k_pair_size takes 42, bounded at 64 (8 waves per SIMD: it waits for memory); k_pair_write carries the block function with the three scans and the
column search and takes 115, bounded at 128 = 4 waves per SIMD, 16 waves per CU, which its 16 640 bytes of LDS per block of four waves (nine
blocks in 160 KB) allow as well.  LDS: k_pair_size declares the 16 u64 of the block scan, k_pair_write four windows of ROWS_WINDOW bytes and 16
dwords each."""
from test_kernel_resources import _find, _kernel_isa, _kernel_metadata

WINDOW = 4096
DECLARED = {"k_pair_size": (16 * 8, 64), "k_pair_write": (4 * (WINDOW + 64), 128)}


def test_the_pairwise_kernels_use_no_scratch_and_only_the_lds_they_declare():
    md = _kernel_metadata()
    assert len(_find(md, "k_pair_")) == 2
    for name, (lds, vgpr) in DECLARED.items():
        found = _find(md, name)
        assert len(found) == 1, name
        for k in found:
            assert k["scratch"] == 0 and k["spill"] == 0, (name, k)
            assert k["vgpr"] <= vgpr, (name, k)
            assert k["lds"] == lds, (name, k)


def test_the_write_kernel_stores_dwords_and_has_no_atomics():
    isa = _kernel_isa("k_pair_write", "")
    assert any(i.startswith("global_store_dword") for i in isa)
    assert any(i.startswith("ds_write_b8") for i in isa)      # blocks are put together in LDS
    assert any(i.startswith("ds_bpermute_b32") for i in isa)                                   # the column search goes over the lanes
    assert not any(i.startswith(("global_atomic", "flat_atomic", "ds_add", "ds_cmpst", "buffer_atomic")) for i in isa)
    assert not any(i.startswith(("scratch_", "buffer_store", "buffer_load")) for i in isa)
