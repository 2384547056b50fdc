"""CPU: what the compiler made of the kernels of csrc/smr_rows.hpp, read from the gfx950 code object inside libsmr_hip.so (no GPU needed), in
the manner of test_kernel_resources.py.  None of them may use scratch or spill a vector register.  Registers, from what the build gives:
k_rows_stat, k_rows_size and k_rows_fmt stay within 64 (8 waves per SIMD: they wait for memory); the two instantiations of k_rows_write carry a
whole row function with the 128-bit arithmetic of the number formatter and take 102 / 107, bounded at 128 = 4 waves per SIMD, 16 waves per
CU, which their 16 640 bytes of LDS per block of four waves (nine blocks in 160 KB) allow as well.  LDS: k_rows_size declares the 16 u64 of
the block scan, k_rows_write four windows of ROWS_WINDOW bytes and 16 dwords each, the others none."""
from test_kernel_resources import _find, _kernel_isa, _kernel_metadata

WINDOW = 4096
DECLARED = {"k_rows_stat": (0, 64), "k_rows_size": (16 * 8, 64), "k_rows_fmt": (0, 64), "k_rows_write": (4 * (WINDOW + 64), 128)}


def test_the_rows_kernels_use_no_scratch_and_only_the_lds_they_declare():
    md = _kernel_metadata()
    for name, (lds, vgpr) in DECLARED.items():
        found = _find(md, name)
        assert len(found) == (2 if name == "k_rows_write" else 1), name
        for k in found:
            assert k["scratch"] == 0 and k["spill"] == 0, (name, k)
            assert k["vgpr"] <= vgpr, (name, k)
            assert k["lds"] == lds, (name, k)


def test_the_write_kernel_stores_dwords_and_has_no_atomics():
    for stream in ("ILj0E", "ILj1E"):
        isa = _kernel_isa("k_rows_write", stream)
        assert any(i.startswith("global_store_dword") for i in isa), stream
        assert any(i.startswith("ds_write_b8") or i.startswith("ds_store_b8") for i in isa), stream      # rows are put together in LDS
        assert not any(i.startswith(("global_atomic", "flat_atomic", "ds_add", "ds_cmpst", "buffer_atomic")) for i in isa), stream
        assert not any(i.startswith(("scratch_", "buffer_store", "buffer_load")) for i in isa), stream
