"""GPU (-m gpu): the %id / %coverage pass of libsmr_hip (csrc/smr_idcov.hpp) against what the UNMODIFIED reference left after its
denovo_stats under -otu_map / -de_novo_otu (tests/golden/otu/, written by tests/golden/make_golden_otu.py): per-read records byte for
byte, the four Readstats totals; the kernels at the seam smr_idcov_batch on hand-made triples, on the alignments of 5 kb reads and over
the whole range of the rounding arithmetic; the four sums through smr_counters_accumulate; what the compiler made of the kernels."""
import re

import pytest

import sortmerna_amd as smr
from helpers import otu

gpu = pytest.mark.gpu

CASES = ["syn", "syn_all", "real", "two_db", "syn_denovo_only", "syn_multipart"]


@pytest.fixture(scope="module")
def engine():
    e = smr.Engine(0)      # raises without a GPU / without the HIP library: no CPU fallback
    yield e
    e.close()


@gpu
@pytest.mark.parametrize("case", CASES)
def test_records_after_the_pass_equal_the_reference_after_denovo_stats(engine, case, tmp_path):
    otu.body_records_and_totals(engine, case, tmp_path)


@gpu
def test_the_same_under_the_dfs_seed_kernel(engine, tmp_path):
    engine.set_seed_mode(1)
    try:
        otu.body_records_and_totals(engine, "syn_all", tmp_path)
    finally:
        engine.set_seed_mode(0)


@gpu
def test_without_the_pass_the_four_counters_are_zero(engine, tmp_path):
    otu.body_without_the_pass_the_counters_are_zero(engine, "two_db", tmp_path)


@gpu
def test_pass_before_traceback_is_a_state_error_and_thresholds_are_checked(engine, tmp_path):
    otu.body_pass_before_traceback_is_a_state_error(engine, "syn", tmp_path)


@gpu
def test_handmade_triples_through_the_seam(engine):
    otu.body_handmade_triples(engine)


@gpu
def test_alignments_of_5kb_reads_against_the_host_walk(engine, tmp_path):
    """hundreds of operations per CIGAR (k_idcov_many) and the occasional short one; n_miss / n_gap / n_match and the class against
    Read::calc_miss_gap_match restated on the host"""
    classes = otu.body_long_reads(engine, tmp_path)
    assert len(classes) >= 2, classes


@gpu
def test_rounding_arithmetic_equals_ieee_doubles_without_contraction(engine):
    """every n_tot in 1 .. 600 and every n_match <= n_tot (180 900 triples), plus every n_match for five n_tot between 4 000 and 6 000 (the
    5 kb regime), under six thresholds: the class equals floor(x * 1000.0 + 0.5) / 1000.0 >= t evaluated in Python floats, where the product
    and the sum round separately as in the reference's host code (hipcc would fuse them if the kernel let it).
    What this half pins is the ARITHMETIC on the device (division, conversion, floor, compare, class order) over the whole range; it cannot tell a
    fused from an unfused build for n_tot <= 2000, where both give the same floor, and nobody has shown that it can at 4 000 - 6 000.  That the
    build is unfused is pinned by the code-object test below."""
    assert otu.body_arithmetic(engine, range(1, 601)) == 180900
    assert otu.body_arithmetic(engine, (4000, 4507, 5000, 5531, 6000)) == 4000 + 4507 + 5000 + 5531 + 6000 + 5


@gpu
def test_counters_accumulate_carries_the_four_sums_over_two_batches(engine, tmp_path):
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")           # plain device memory of the caller's own, as a host's block of sums is
    hip.hipMalloc.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t]
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipFree.argtypes = [ctypes.c_void_p]
    held = []

    def device_zeros(n):
        p = ctypes.c_void_p()
        assert hip.hipMalloc(ctypes.byref(p), 8 * n) == 0 and hip.hipMemset(p, 0, 8 * n) == 0 and hip.hipDeviceSynchronize() == 0
        held.append(p)
        return (p, n), p.value

    def to_host(acc):
        p, n = acc
        h = (ctypes.c_uint64 * n)()
        assert hip.hipMemcpy(h, p, 8 * n, 2) == 0          # hipMemcpyDeviceToHost
        return [int(x) for x in h]

    try:
        otu.body_accumulate_carries_the_four_sums(engine, tmp_path, device_zeros, to_host)
    finally:
        for p in held:
            hip.hipFree(p)


@gpu
def test_the_pass_has_its_own_profile_family(engine, tmp_path):
    engine.prof_reset()
    _, _, keep = otu.run(engine, "syn", tmp_path)
    otu.free(keep)
    k = engine.prof_kernels()
    assert "k_idcov" in k and k["k_idcov"]["launches"] == 1 and k["k_idcov"]["ms"] > 0, k.get("k_idcov")


def test_kernels_of_the_pass_use_no_scratch_and_keep_the_rounding_unfused():
    """from the gfx950 code object (no GPU needed): no scratch, no spilled registers, and at most 128 VGPRs -- four waves per SIMD, the budget
    tests/test_kernel_resources.py gives the other stand-alone one-wave-per-block kernels (the pass lives on loads in flight, not on
    arithmetic); and in each of the two kernels two v_add_f64 next to two v_floor_f64 -- the two `+ 0.5`, which a contracted build would
    have folded into v_fma_f64"""
    from test_kernel_resources import _find, _kernel_isa, _kernel_metadata
    md = _kernel_metadata()
    for name in ("k_idcov_collect", "k_idcov_few", "k_idcov_many", "k_idcov_gather"):
        for k in _find(md, name):
            assert k["scratch"] == 0 and k["spill"] == 0 and k["vgpr"] <= 128, (name, k)
    for name in ("k_idcov_few", "k_idcov_many"):
        for k in _find(md, name):
            assert k["lds"] == 0, (name, k)
        isa = _kernel_isa(name)
        assert sum(1 for i in isa if i.startswith("v_add_f64")) == 2 and sum(1 for i in isa if i.startswith("v_floor_f64")) == 2, name
        # and what each v_floor_f64 reads is the result of a v_add_f64, not of a fused multiply-add (whatever order the scheduler chose)
        last_writer = {}
        for ins in isa:
            m = re.match(r"(v_\w+)\s+(v\[\d+:\d+\])(?:,\s*(v\[\d+:\d+\]))?", ins)
            if not m:
                continue
            if m.group(1).startswith("v_floor_f64"):
                assert last_writer.get(m.group(3), "").startswith("v_add_f64"), (name, ins, last_writer.get(m.group(3)))
            last_writer[m.group(2)] = m.group(1)
    assert any(i.startswith("v_add_u32_dpp") for i in _kernel_isa("k_idcov_many"))       # the scan of the operation lengths


# ---- the files, written from the records the DEVICE produced ---------------------------------------------------------------------------

def _files_from_device_records(engine, reads_text, recs, parts_per_db, out_dir, min_id, min_cov):
    from sortmerna_amd import report
    rep = report.Report(str(out_dir), is_fastq=False, fastx=False, other=False, otu_map=True, denovo=True, min_id=min_id, min_cov=min_cov)
    for k, parts in enumerate(parts_per_db):
        for j, ix in enumerate(parts):
            rep.set_part(k, j, ix)
    for (hdr, seq, qual), rec in zip(reads_text, recs):
        rep.add(hdr, seq, None, rec)
    rep.close()
    return rep.total_otu


@gpu
@pytest.mark.parametrize("case", ["syn", "two_db", "syn_multipart", "real"])
def test_files_written_from_device_records_equal_the_reference_files(engine, case, tmp_path):
    import os
    from helpers import fastx, golden
    g = otu.load()[case]
    recs, _, keep = otu.run(engine, case, tmp_path)
    try:
        idx, _, _ = keep
        out = tmp_path / "out"
        out.mkdir()
        n = _files_from_device_records(engine, fastx.read_fastx(golden.inputs(g["inputs"])[1]), recs, [d["parts"] for d in idx], out, g["min_id"], g["min_cov"])
    finally:
        otu.free(keep)
    assert n == g["n_groups"] and os.path.isfile(out / "otu_map.txt") == (g["otu_map"] is not None)
    if g["otu_map"]:
        assert open(out / "otu_map.txt", "rb").read() == open(os.path.join(otu.OTU_DIR, g["otu_map"]), "rb").read()
    assert open(out / "aligned_denovo.fa", "rb").read() == open(os.path.join(otu.OTU_DIR, case + ".denovo.fa"), "rb").read()


@gpu
@pytest.mark.parametrize("run", ["default", "id90_cov50"])
def test_config2_at_full_size_through_the_gz_front_end(run, tmp_path):
    """BASELINE config 2 -- the reference's 100 000 amplicon reads against silva-arc-16s-id95, straight from the .gz -- under -otu_map -de_novo_otu
    (tests/golden/config2/config2_otu.json, written by make_golden_config2_otu.py from the unmodified reference): the records after the pass through
    MD5 digests per 1000 reads, the four totals, and the MD5 of otu_map.txt and aligned_denovo.fa written from the device's records.  ~50 000
    alignments: the work list of k_idcov_few spans dozens of blocks of the collector."""
    import gzip
    import hashlib
    import json
    import os
    from helpers import paths
    from test_gpu_config2_fullsize import digests
    c2 = os.path.join(paths.GOLDEN, "config2")
    base = json.load(open(os.path.join(c2, "config2.json")))
    g = json.load(open(os.path.join(c2, "config2_otu.json")))
    r = g["runs"][run]
    db = os.path.join(str(tmp_path), base["db"][:-3])
    with gzip.open(os.path.join(c2, base["db"]), "rb") as f, open(db, "wb") as o:
        o.write(f.read())
    e = smr.Engine(0)
    try:
        parts = smr.Index.build_gpu(e, db, 18, 3072.0, 10000)
        reads = smr.Reads.from_fastx_text(os.path.join(c2, base["reads"]), 0)
        assert reads.count == g["n_reads"]
        assert smr.minimal_score(r["lambda"], r["K"], parts[0].info(), reads.count, reads.total_len) == r["minimal_score"]
        p = smr.default_params(minimal_score=r["minimal_score"])
        smr.align(e, reads, [parts], [p], with_cigar=True, id_cov=(r["min_id"], r["min_cov"]))
        recs = e.records()
        tot = e.idcov_counters()
        assert [tot["n_yid_ycov"], tot["n_yid_ncov"], tot["n_nid_ycov"], tot["num_denovo"]] == r["totals"]
        assert e.counters(1)["num_aligned"] == r["num_aligned"] and sum(1 for x in recs if x) == r["n_records"]
        total, chunks = digests(recs, g["chunk"])
        bad = [k for k, (a, b) in enumerate(zip(chunks, r["md5_chunks"])) if a != b]
        assert not bad, "%d of %d chunks of %d reads differ from the reference's records after denovo_stats; first: reads %d.." % (len(bad), len(chunks), g["chunk"], bad[0] * g["chunk"])
        assert total == r["md5_total"]
        out = tmp_path / "out"
        out.mkdir()
        n = _files_from_device_records(e, (reads.record_text(i) for i in range(reads.count)), recs, [parts], out, r["min_id"], r["min_cov"])
        md5 = lambda q: hashlib.md5(open(q, "rb").read()).hexdigest()
        assert n == r["n_groups"] and os.path.isfile(out / "otu_map.txt") == (r["md5_otu_map"] is not None)
        if r["md5_otu_map"]:
            assert md5(out / "otu_map.txt") == r["md5_otu_map"]
        assert md5(out / "aligned_denovo.fa") == r["md5_denovo"]
    finally:
        e.close()
