"""CPU: what the compiler made of k_sw16h<19> (smr_walk.hpp, the packed-f16 flavour of k_sw16), read from the gfx950 code object inside
libsmr_hip.so like tests/test_kernel_resources.py reads k_sw16<19>: the integer kernel's register and spill bounds, no scratch access inside a
step loop, and the instruction count the flavour exists for -- the score-only step loop without N holds 8 packed instructions per cell pair
(perm, a = diag + T, E - ge, e = max3, F - ge, f = max3(., uy, uy), h = max3, y = h - go) and one three-operand maximum per two rows for the
running maximum: 4 x (8 x 19 + 10) = 648 per period of four steps against the integer loop's 4 x 10 x 19 = 760.  A canonicalising
instruction in front of a maximum (v_pk_mul_f16 x, 1.0, or v_pk_max_f16 x, x) would give the gain back."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from sortmerna_amd import build

LLVM = "/opt/rocm/lib/llvm/bin"
KERNEL = "k_sw16hILi19"
R = 19


def _code_object(d):
    bundler = os.path.join(LLVM, "clang-offload-bundler")
    if not (os.path.exists(bundler) and os.path.exists(os.path.join(LLVM, "llvm-objdump")) and os.path.exists(os.path.join(LLVM, "llvm-readelf")) and shutil.which("objcopy")):
        pytest.skip("ROCm LLVM tools not installed")
    lib = build.build_library()
    fat, co = os.path.join(d, "fatbin"), os.path.join(d, "gfx950.o")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
    subprocess.check_call([bundler, "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + co, "--unbundle"])
    return co


@pytest.fixture(scope="module")
def kernel():
    """-> (metadata of the kernel, its instructions as (address, text, branch target or None))"""
    with tempfile.TemporaryDirectory() as d:
        co = _code_object(d)
        notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co]).decode()
        text = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", co]).decode()
    md = None
    for blk in re.split(r"\n  - \.agpr_count", notes)[1:]:
        if KERNEL in re.search(r"\.name:\s+(\S+)", blk).group(1):
            f = lambda key: int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))   # noqa: E731
            md = dict(vgpr=f("vgpr_count"), spill=f("vgpr_spill_count"), scratch=f("private_segment_fixed_size"))
    assert md, "kernel %s not in the code object" % KERNEL
    isa, on, base = [], False, 0
    for line in text.splitlines():
        m = re.match(r"^([0-9a-f]+) <(\S+)>:", line)
        if m:
            on, base = KERNEL in m.group(2), int(m.group(1), 16)
            continue
        if on and line.strip():
            ins, _, rest = line.partition("//")
            a = re.match(r"\s*([0-9A-Fa-f]+):", rest)
            t = re.search(r"<\S+\+0x([0-9a-f]+)>\s*$", rest) if ins.strip().startswith(("s_cbranch", "s_branch")) else None
            isa.append((int(a.group(1), 16), ins.strip(), base + int(t.group(1), 16) if t else None))
    assert isa
    return md, isa


def _step_loops(isa):
    """the innermost loops that hold a period of four steps: the instructions between a backward branch and its target, with at least
    4 x 19 three-operand maxima and no such loop inside; six of them (keys / score only / prefix, each with and without N)"""
    loops = []
    for addr, ins, target in isa:
        if target is not None and target <= addr:
            body = [i for a, i, _ in isa if target <= a <= addr]
            if sum(1 for i in body if i.startswith("v_pk_maximum3_f16")) >= 4 * R:
                loops.append((target, addr, body))
    inner = [lp for lp in loops if not any(o is not lp and lp[0] <= o[0] and o[1] <= lp[1] for o in loops)]
    return [body for _, _, body in inner]


def test_registers_spills_and_no_scratch_access_between_the_maxima_of_a_step_loop(kernel):
    md, isa = kernel
    assert md["vgpr"] <= 168 and md["spill"] <= 96, md
    runs, stretch = [], 0
    for _, ins, _ in isa + [(0, "scratch_end", None)]:
        if ins.startswith("scratch_"):
            runs.append(stretch); stretch = 0
        elif ins.startswith("v_pk_maximum3_f16"):
            stretch += 1
    total = sum(runs)
    # (a period of the cheapest loop holds 4 x (3 x 19 + 10) maxima, of the others 4 x 3 x 19)
    assert total >= 6 * 4 * 3 * R and sum(r for r in runs if r >= 4 * 3 * R) == total, (total, [r for r in runs if r])
    assert len(_step_loops(isa)) == 6


def test_the_score_only_step_loop_holds_eight_packed_instructions_per_cell_pair(kernel):
    _, isa = kernel
    loops = _step_loops(isa)
    packed = lambda body: sum(1 for i in body if i.startswith("v_pk_") or i.startswith("v_perm_b32"))   # noqa: E731
    counts = sorted(packed(b) for b in loops)
    print("v_pk_* + v_perm_b32 per period of the six step loops:", counts, "instructions per period:", sorted(len(b) for b in loops))
    no_n = [b for b in loops if not any(i.startswith("v_bfi") for i in b)]      # (HASN replaces the looked-up value with one v_bfi_b32 per cell pair)
    assert len(no_n) == 3
    # the variant with end cells keeps its keys with 32-bit maxima; the other two are the score-only loop and the prefix loop, whose R running
    # maxima the compiler also updates with three-operand maxima (two steps at a time): the bound holds for both
    plain = [b for b in no_n if not any(i.startswith(("v_max_u32", "v_max3_u32")) for i in b)]
    assert len(plain) == 2
    for body in plain:
        assert packed(body) <= 650, counts                  # 4 x (8 x 19 + 10) = 648


def test_no_canonicalising_instruction_in_the_step_loops(kernel):
    _, isa = kernel
    for body in _step_loops(isa):
        assert not any(i.startswith("v_pk_mul_f16") for i in body)
        for i in body:
            if i.startswith("v_pk_max_f16"):
                ops = [o.strip() for o in i.split(None, 1)[1].split(",")]
                assert not (len(ops) >= 3 and ops[1] == ops[2].split()[0]), i
    # (and the integer flavour's instructions stay in the integer kernel)
    assert not any(i.startswith("v_pk_max_i16") for _, i, _ in isa)
