"""CPU: what the compiler made of k_mates_zip (csrc/smr_mates.hpp), read from the gfx950 code object inside libsmr_hip.so (no GPU needed), in the
manner of test_rows_kernel_resources.py.  The kernel may use no scratch and spill nothing; it declares no LDS, so it has none.  Registers: the
build gives 44 vector registers; the bound is 64 = 8 waves per SIMD, which a kernel that waits for memory should keep.  The output is
stored as whole dwords (and, at the ends of a team's range, as bytes); there are no atomics."""
from test_kernel_resources import _find, _kernel_isa, _kernel_metadata


def test_the_interleave_kernel_uses_no_scratch_no_lds_and_few_registers():
    found = _find(_kernel_metadata(), "k_mates_zip")
    assert len(found) == 1
    k = found[0]
    assert k["scratch"] == 0 and k["spill"] == 0, k
    assert k["lds"] == 0, k
    assert k["vgpr"] <= 64, k


def test_the_interleave_kernel_stores_dwords_and_has_no_atomics():
    isa = _kernel_isa("k_mates_zip")
    assert any(i.startswith("global_store_dword") for i in isa)
    assert any(i.startswith("global_store_byte") for i in isa)          # the shared dwords at the ends of a team's range
    assert any(i.startswith("v_perm_b32") for i in isa)                 # the byte funnel
    assert not any(i.startswith(("global_atomic", "flat_atomic", "ds_", "buffer_atomic")) for i in isa)
    assert not any(i.startswith(("scratch_", "buffer_store", "buffer_load")) for i in isa)
