"""CPU: what the compiler made of the kernels of csrc/smr_fxsplit.hpp, read from the gfx950 code object inside libsmr_hip.so (no GPU needed),
in the manner of test_kernel_resources.py.  None of them may use scratch or spill or more than 64 vector registers.  LDS: k_fxs_measure
declares the wave sums of its eight scans (8 streams x 16 waves x 8 bytes), k_fxs_scan the 16 u64 of the block scan, k_fxs_copy none -- a
team keeps the open dword of its output in registers."""
from test_kernel_resources import _find, _kernel_isa, _kernel_metadata

DECLARED_LDS = {"k_fxs_measure": 8 * 16 * 8, "k_fxs_scan": 16 * 8, "k_fxs_copy": 0}


def test_the_split_kernels_use_no_scratch_and_only_the_lds_they_declare():
    md = _kernel_metadata()
    for name, lds in DECLARED_LDS.items():
        found = _find(md, name)
        assert found, name
        for k in found:
            assert k["scratch"] == 0 and k["spill"] == 0, (name, k)
            assert k["vgpr"] <= 64, (name, k)                   # (8 waves per SIMD: these kernels wait for memory)
            assert k["lds"] == lds, (name, k)


def test_the_text_is_read_as_dwords_and_the_output_is_stored_as_dwords():
    for name in ("k_fxs_measure", "k_fxs_copy"):
        assert any(i.startswith(("global_load_dwordx4", "global_load_dword")) for i in _kernel_isa(name)), name
    copy = _kernel_isa("k_fxs_copy")
    assert any(i.startswith("global_store_dword") for i in copy)
    assert not any(i.startswith(("global_atomic", "flat_atomic")) for i in copy)
