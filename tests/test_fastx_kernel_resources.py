"""CPU: what the compiler made of the kernels of csrc/smr_fastx.hpp, read from the gfx950 code object inside libsmr_hip.so (no GPU needed),
in the manner of test_kernel_resources.py.  None of them may use scratch or spill; k_fx_pack puts its words together in registers and
declares no LDS, the line and record kernels declare 16 words for the block scan (+ two words of block-wide minimum / maximum)."""
from test_kernel_resources import _find, _kernel_isa, _kernel_metadata

KERNELS = ["k_fx_count", "k_fx_scan", "k_fx_lines", "k_fx_classify", "k_fx_records", "k_fx_reclen", "k_fx_pack"]


def test_the_fastx_kernels_use_no_scratch_and_only_the_lds_they_declare():
    md = _kernel_metadata()
    for name in KERNELS:
        for k in _find(md, name):
            assert k["scratch"] == 0 and k["spill"] == 0, (name, k)
            assert k["vgpr"] <= 64, (name, k)                   # (8 waves per SIMD: these kernels wait for memory)
    declared = {"k_fx_count": 64, "k_fx_scan": 64, "k_fx_lines": 64, "k_fx_classify": 64 + 8, "k_fx_records": 0, "k_fx_reclen": 64 + 8, "k_fx_pack": 0}
    for name, lds in declared.items():
        for k in _find(md, name):
            assert k["lds"] == lds, (name, k)


def test_the_text_is_read_as_dwordx4_and_the_words_are_stored_whole():
    assert any(i.startswith("global_load_dwordx4") for i in _kernel_isa("k_fx_count"))
    assert any(i.startswith("global_load_dwordx4") for i in _kernel_isa("k_fx_lines"))
    pack = _kernel_isa("k_fx_pack")
    assert not any(i.startswith(("global_atomic", "flat_atomic", "global_store_byte", "global_store_short")) for i in pack)
    assert sum(1 for i in pack if i.startswith("global_store_dword")) >= 3
