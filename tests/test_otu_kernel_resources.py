"""CPU: what the compiler made of the kernels of csrc/smr_otu.hpp and of k_fxs_dn_measure (csrc/smr_fxsplit.hpp), read from the gfx950 code
object inside libsmr_hip.so (no GPU needed), in the manner of test_rows_kernel_resources.py.  None of them may use scratch or spill a vector
register.  Registers are pinned at what the build gives (the numbers DESIGN.md quotes), and that number is bounded by the occupancy meant: k_otu_classify carries the two walks of the pass and takes 80, bounded at 96 = 5 waves per
SIMD; everything else waits for memory and stays within 64 (8 waves per SIMD).  LDS: the two sizing kernels declare the 16 u64 of the block
scan, k_otu_hist a row of 256 counters for each of its four waves, k_otu_move three such rows and a stage of 1024 keys and 1024 values per wave (44 KB), k_otu_write four windows of ROWS_WINDOW bytes and 16 dwords
each, k_fxs_dn_measure the wave sums of its four scans (4 streams x 16 waves x 8 bytes), the others none."""
import re

from test_kernel_resources import _find, _kernel_isa, _kernel_metadata

WINDOW = 4096
# name: (LDS bytes, VGPR bound, VGPRs of the build this was written against)
DECLARED = {"k_otu_classify": (0, 96, 80), "k_otu_size": (16 * 8, 64, 42), "k_otu_pairs": (0, 64, 16), "k_otu_hist": (4 * 256 * 4, 64, 28),
            "k_otu_move": (3 * 4 * 256 * 4 + 2 * 4 * 1024 * 4, 64, 32), "k_otu_iota": (0, 64, 4), "k_otu_wsize": (16 * 8, 64, 46), "k_otu_write": (4 * (WINDOW + 64), 64, 59),
            "k_otu_groups": (0, 64, 14), "k_otu_gcount": (0, 64, 6), "k_fxs_dn_measure": (4 * 16 * 8, 64, 34)}


def test_the_otu_kernels_use_no_scratch_and_only_the_lds_they_declare():
    md = _kernel_metadata()
    for name, (lds, vgpr, built) in DECLARED.items():
        found = _find(md, name)
        assert len(found) == 1, name
        for k in found:
            assert k["scratch"] == 0 and k["spill"] == 0, (name, k)
            assert k["vgpr"] == built, (name, k)                # pinned at what the build gives (DESIGN.md section 3 quotes these)
            assert built <= vgpr, name                          # ... which stays within the occupancy the kernel is meant for
            assert k["lds"] == lds, (name, k)


def test_the_sort_and_the_writer_have_no_atomics():
    """placement is by ballots, scans and one counter per digit and wave in LDS that a single lane moves on: a hot reference costs what an
    even spread costs"""
    for name in ("k_otu_hist", "k_otu_move", "k_otu_wsize", "k_otu_write", "k_otu_pairs", "k_otu_groups"):
        isa = _kernel_isa(name)
        assert not any(i.startswith(("global_atomic", "flat_atomic", "ds_add", "ds_cmpst", "buffer_atomic")) for i in isa), name
        assert not any(i.startswith(("scratch_", "buffer_store", "buffer_load")) for i in isa), name
    write = _kernel_isa("k_otu_write")
    assert any(i.startswith("global_store_dword") for i in write)
    assert any(i.startswith("ds_write_b8") or i.startswith("ds_store_b8") for i in write)             # the ids are put together in LDS
    assert any(i.startswith("v_add_u32_dpp") for i in _kernel_isa("k_otu_classify"))                   # the scan of the operation lengths


def test_the_classify_kernel_keeps_the_rounding_unfused():
    """two v_add_f64 next to two v_floor_f64 -- the two `+ 0.5`, which a contracted build would have folded into v_fma_f64 -- and what each
    v_floor_f64 reads is the result of a v_add_f64 (the check test_gpu_idcov.py makes for the pass)"""
    isa = _kernel_isa("k_otu_classify")
    assert sum(1 for i in isa if i.startswith("v_add_f64")) == 2 and sum(1 for i in isa if i.startswith("v_floor_f64")) == 2
    last_writer = {}
    for ins in isa:
        m = re.match(r"(v_\w+)\s+(v\[\d+:\d+\])(?:,\s*(v\[\d+:\d+\]))?", ins)
        if not m:
            continue
        if m.group(1).startswith("v_floor_f64"):
            assert last_writer.get(m.group(3), "").startswith("v_add_f64"), (ins, last_writer.get(m.group(3)))
        last_writer[m.group(2)] = m.group(1)
    # and the rounded value is scaled back by a product (`* 0.001`), not by a division: one v_mul_f64 reads each v_floor_f64's result
    floors = [re.match(r"v_floor_f64\S*\s+(v\[\d+:\d+\])", i).group(1) for i in isa if i.startswith("v_floor_f64")]
    for reg in floors:
        assert any(i.startswith("v_mul_f64") and reg in i.split(None, 1)[1].split(",", 1)[1] for i in isa), reg
