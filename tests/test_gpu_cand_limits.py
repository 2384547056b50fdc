"""The candidate stage (k_cand -> k_wlist -> k_walk / k_wnext, k_chain<EXT = false | true>, the retry ladder of smr_align_part) at its path
boundaries and capacity limits.  Every case is a crafted workload (helpers/candcase.py) that first proves, from numbers the ORACLE's unit
entry points give, that its reads land on the side of a limit they are meant for; then the engine runs it, and records, num_aligned, per_db,
n_hit and n_sw_fwd must equal the oracle's.  On single-launch runs (one strand, equal strides) the way every read took -- smr_cand_routes, a
test seam -- must equal what the host model derives from those numbers.

The limits as read from the kernels and confirmed here: a record of k_cand holds <= 64 positions of a read with <= 64 hits and needs room in
its block's 8 192-word slice; k_walk gathers 65..128 positions itself; the LDS set of k_chain<false> holds 384 members, the global one of
k_chain<true> 49 152 (3/4 of 512 / 65 536 slots; a member = a reference that occurs at least twice among the read's positions); the 49 153rd
is SMR_ERR_CAPACITY.  The probe loop of chain_build_set is bounded by the table's slots, so it ends on a full table.

test_emu_cand_limits.py runs the same bodies on the emulator."""
import collections

import pytest

import sortmerna_amd as smr
from helpers import candcase as cc
from helpers.workload import Workload
from test_gpu_parity import _compare

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("mode", [0, 1], ids=["pg", "dfs"])


def _engine(mode=0):
    e = smr.Engine(0)
    e.set_seed_mode(mode)
    e.cand_info_enable(True)
    return e


def _run(e, w, what, stride=None, max_alignments_per_read=None, **opts):
    """engine against oracle: records and the five counters; returns (routes, cand_info) of the run"""
    kw = dict(opts)
    if stride is not None:
        kw.update(is_reverse=0, skiplengths=[stride, stride, stride])      # one strand, equal strides: one launch sees every searchable read
    recs_o, ctr_o = w.oracle_records(**kw)
    e.prof_reset()
    p = smr.default_params(minimal_score=w.minimal_score, **kw)
    smr.align(e, w.reads, [w.parts], [p], max_alignments_per_read=max_alignments_per_read)
    recs_g, ctr_g, prof = e.records(), e.counters(1), e.prof()
    got = dict(num_aligned=ctr_g["num_aligned"], per_db=ctr_g["reads_matched_per_db"][0], n_hit=prof.n_hit, n_sw_fwd=prof.n_sw_fwd)
    exp = {k: ctr_o[k] for k in got}
    print("%s: engine %s, oracle %s, ladder %s" % (what, got, exp, e.cand_info()))
    _compare(recs_g, recs_o, what)
    assert got == exp, (what, got, exp)
    return e.cand_routes(), e.cand_info()


def _check_routes(w, nums, routes, what, **model):
    marked = [bool(r) for r in routes]
    for i, x in enumerate(nums):
        assert marked[i] or x["ncand"] == 0, "%s: read %d (%s) has %d candidates and was not marked" % (what, i, w.tags[i], x["ncand"])
    exp = cc.expected_routes(nums, marked, **model)
    bad = [(i, w.tags[i], int(routes[i]), exp[i], nums[i]) for i in range(len(nums)) if marked[i] and exp[i] is not None and routes[i] != exp[i]]
    assert not bad, "%s: %d reads took another way than the host model's (read, tag, device, host, numbers): %s" % (what, len(bad), bad[:4])
    return exp


def _ordinary(tmp_path):
    d = tmp_path / "ordinary"
    d.mkdir(exist_ok=True)
    return Workload(str(d), db_nt=60_000, n_reads=300, seed=31)


def _numbers(w, stride):
    hx = cc.HostIndex(w)
    try:
        return [hx.numbers(s, stride) for s in w.seqs]
    finally:
        hx.close()


# ------------------------------------------------------------------------------------------------ a. position counts
POSITION_VARIANTS = [{}, {"SMR_WALK_GATHER": "0"}, {"SMR_HANDOVER": "0"}]


def position_counts_body(tmp_path, monkeypatch, stride, env, mode):
    w = cc.positions_workload(str(tmp_path), stride)
    nums = _numbers(w, stride)
    by = collections.Counter(x["npos"] for x in nums if x["nh"] <= cc.CAND_HITS and x["ncand"] > 0)
    for t in cc.POSITION_VALUES:
        assert by[t] >= 8, "stride %d: %d reads with %d positions (wanted >= 8); %s" % (stride, by[t], t, sorted(by.items()))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    e = _engine(mode)
    try:
        routes, info = _run(e, w, "positions, stride %d, %s" % (stride, env), stride=stride)
        assert 1 <= info["attempts"] <= 1 + sum(info["retries"].values()) and not info["chain_ext"]
        gather, handover = env.get("SMR_WALK_GATHER") != "0", env.get("SMR_HANDOVER") != "0"
        exp = _check_routes(w, nums, routes, "positions", gather=gather, handover=handover)
        # what the model says at the boundaries, spelled out
        for i, x in enumerate(nums):
            if x["ncand"] and x["nh"] <= cc.CAND_HITS and x["npos"] in cc.POSITION_VALUES:
                want = cc.ROUTE_CHAIN if not handover else cc.ROUTE_RECORD if x["npos"] <= 64 else cc.ROUTE_GATHER if (x["npos"] <= 128 and gather) else cc.ROUTE_CHAIN
                assert exp[i] == want == routes[i], (i, x, exp[i], want, routes[i])
    finally:
        e.close()


@MODES
@pytest.mark.parametrize("env", POSITION_VARIANTS, ids=["default", "gather0", "handover0"])
@pytest.mark.parametrize("stride", [18, 3])
def test_reads_with_63_to_257_positions_take_the_way_the_host_model_says(tmp_path, monkeypatch, stride, env, mode):
    position_counts_body(tmp_path, monkeypatch, stride, env, mode)


# ------------------------------------------------------------------------------------------------ b. hit counts
def hit_counts_body(tmp_path, mode=0):
    w = cc.hits_workload(str(tmp_path))
    nums = _numbers(w, 3)
    by = collections.Counter((x["nh"], x["npos"]) for x in nums)
    assert by[(64, 64)] >= 8 and by[(65, 65)] >= 8 and by[(63, 63)] >= 8, by
    e = _engine(mode)
    try:
        routes, _ = _run(e, w, "64 / 65 hits", stride=3)
        _check_routes(w, nums, routes, "hits")
        for i, x in enumerate(nums):
            if x["nh"] in (63, 64):
                assert routes[i] == cc.ROUTE_RECORD, (i, x, routes[i])
            if x["nh"] == 65:
                assert routes[i] == cc.ROUTE_CHAIN, (i, x, routes[i])
    finally:
        e.close()


def test_reads_with_64_and_65_seed_hits(tmp_path):
    hit_counts_body(tmp_path)


# ------------------------------------------------------------------------------------------------ c. slice overflow
def slice_overflow_body(tmp_path, monkeypatch, gather, mode):
    w = cc.slice_workload(str(tmp_path))
    nums = _numbers(w, 3)
    assert all(x["nh"] == 17 and x["npos"] == 17 and x["ncand"] == 1 for x in nums), collections.Counter((x["nh"], x["npos"], x["ncand"]) for x in nums)
    assert 3 * 17 * 160 <= cc.CAND_BLOCK * cc.CAND_REC_WORDS < 3 * 17 * 160 + 3 * 17        # ten groups of sixteen fit, no read after them
    if not gather:
        monkeypatch.setenv("SMR_WALK_GATHER", "0")
    e = _engine(mode)
    try:
        routes, _ = _run(e, w, "slice overflow, gather %d" % gather, stride=3)
        exp = _check_routes(w, nums, routes, "slice", gather=gather)
        assert None not in exp
        lost = cc.ROUTE_GATHER if gather else cc.ROUTE_CHAIN
        assert list(routes[:160]) == [cc.ROUTE_RECORD] * 160 and list(routes[160:256]) == [lost] * 96, collections.Counter(routes[:256].tolist())
        assert list(routes[256:]) == [cc.ROUTE_RECORD] * 100          # the second block has its own slice
    finally:
        e.close()


@MODES
@pytest.mark.parametrize("gather", [1, 0], ids=["gather", "gather0"])
def test_a_block_whose_records_outgrow_its_slice(tmp_path, monkeypatch, gather, mode):
    slice_overflow_body(tmp_path, monkeypatch, gather, mode)


# ------------------------------------------------------------------------------------------------ d. LIS variant
def lis_variant_body(tmp_path, mode=0):
    w = cc.lis_workload(str(tmp_path))
    n6, n3 = _numbers(w, 6), None
    serial = [i for i, x in enumerate(n6) if w.tags[i] == "tandem" and 65 <= x["first_window_pairs"] <= 80 and x["npos"] <= cc.WK_MAX_POS and x["nh"] <= cc.CAND_HITS and x["lis_strict"]]
    swapped = [i for i, x in enumerate(n6) if w.tags[i] == "swapped" and x["ncand"] == 1 and x["max_pairs"] >= 30]
    assert len(serial) >= 8 and len(swapped) >= 6, (len(serial), len(swapped), [(x["first_window_pairs"], x["npos"], x["nh"]) for x in n6])
    # reads on which a run of EQUAL read positions would be long enough and the strictly increasing one is not: the oracle makes no Smith-Waterman call for them
    periodic = [i for i, x in enumerate(n6) if w.tags[i] == "periodic" and x["first_window_pairs"] > cc.WAVE_LIS_MAX and x["npos"] <= cc.WK_MAX_POS and x["nh"] <= cc.CAND_HITS
                and x["ncand"] == 1 and x["lis_len"] < 2 <= x["lis_len_nonstrict"]]
    assert len(periodic) >= 6, [(x["first_window_pairs"], x["npos"], x["nh"], x["ncand"], x["lis_len"], x["lis_len_nonstrict"]) for i, x in enumerate(n6) if w.tags[i] == "periodic"]
    e = _engine(mode)
    try:
        routes, _ = _run(e, w, "LIS variants, stride 6", stride=6)
        _check_routes(w, n6, routes, "lis")
        assert all(routes[i] == cc.ROUTE_GATHER for i in serial + periodic), [int(routes[i]) for i in serial + periodic]     # 65..128 positions: k_walk, and there more than 64 pairs in a window
    finally:
        e.close()
    # the other side: exactly 64 pairs in one window (wave_lis_first at its largest) -- the 64-window reads of the hit-count case
    w2 = cc.hits_workload(str(tmp_path / "w64"), per_value=4)
    n3 = _numbers(w2, 3)
    assert sum(1 for x in n3 if x["first_window_pairs"] == 64 and x["npos"] == 64) >= 4
    e = _engine(mode)
    try:
        _run(e, w2, "64 pairs in one window", stride=3)
    finally:
        e.close()


def test_windows_of_64_and_of_65_to_80_pairs(tmp_path):
    lis_variant_body(tmp_path)


# ------------------------------------------------------------------------------------------------ e. LDS table -> global table
def lds_to_ext_body(tmp_path, mode=0):
    below = cc.family_workload(str(tmp_path), cc.LDS_SET_MEMBERS)
    above = cc.family_workload(str(tmp_path), cc.LDS_SET_MEMBERS + 1)
    nb, na = _numbers(below, 18), _numbers(above, 18)
    fam_b = [i for i, t in enumerate(below.tags) if t.startswith("family")]
    fam_a = [i for i, t in enumerate(above.tags) if t.startswith("family")]
    assert fam_b and all(nb[i]["members_lo"] <= nb[i]["members_hi"] <= cc.LDS_SET_MEMBERS for i in range(len(nb)))
    assert max(nb[i]["members_lo"] for i in fam_b) == cc.LDS_SET_MEMBERS, [nb[i]["members_lo"] for i in fam_b]
    assert max(na[i]["members_lo"] for i in fam_a) == cc.LDS_SET_MEMBERS + 1, [na[i]["members_lo"] for i in fam_a]
    e = _engine(mode)
    try:
        routes, info = _run(e, below, "384 members", stride=18)
        assert info["retries"]["SCAP"] == 0 and not info["chain_ext"] and info["chain_scap"] == 512
        _check_routes(below, nb, routes, "384 members")
        assert all(routes[i] == cc.ROUTE_CHAIN for i in fam_b if nb[i]["npos"] > cc.WK_MAX_POS)
        routes, info = _run(e, above, "385 members", stride=18)
        assert info["retries"]["SCAP"] == 1 and 2 <= info["attempts"] <= 1 + sum(info["retries"].values()) and info["chain_ext"] and info["keys_cap"] >= 65536
        _check_routes(above, na, routes, "385 members", ext=True)
        over = [i for i in fam_a if na[i]["members_lo"] > cc.LDS_SET_MEMBERS]
        assert over and all(routes[i] == cc.ROUTE_CHAIN | cc.ROUTE_EXT for i in over)
        # from then on: no further retry for the same reads, and ordinary reads are what they were
        routes, info = _run(e, above, "385 members again", stride=18)
        assert info["attempts"] == 1 and info["chain_ext"]
        routes, info = _run(e, below, "384 members, global tables on", stride=18)
        assert info["attempts"] == 1 and all(routes[i] == cc.ROUTE_CHAIN for i in fam_b if nb[i]["npos"] > cc.WK_MAX_POS)
        w = _ordinary(tmp_path)
        _run(e, w, "an ordinary batch after the switch")
    finally:
        e.close()


def test_a_set_of_384_members_and_one_of_385(tmp_path):
    lds_to_ext_body(tmp_path)


# ------------------------------------------------------------------------------------------------ f. the PAIRS ladder
def pairs_ladder_body(tmp_path, mode=0):
    w = cc.pairs_workload(str(tmp_path))
    nums = _numbers(w, 18)
    big = [i for i, t in enumerate(w.tags) if t == "pairs"]
    assert max(nums[i]["npos"] for i in big) > cc.PAIRS_CAP0 and all(nums[i]["members_hi"] <= cc.LDS_SET_MEMBERS for i in big), [nums[i] for i in big]
    e = _engine(mode)
    try:
        assert e.cand_info()["pairs_cap"] in (0, cc.PAIRS_CAP0)
        routes, info = _run(e, w, "more tuples than pairs_cap", stride=18)
        assert info["retries"]["PAIRS"] == 1 and info["retries"]["SCAP"] == 0 and 2 <= info["attempts"] <= 1 + sum(info["retries"].values()), info      # (the hit lists of the seed stage may grow in the same calls: one attempt can be redone for two causes)
        assert info["pairs_cap"] == 4 * cc.PAIRS_CAP0 and info["hits_cap"] == 4 * 4096, info
        _check_routes(w, nums, routes, "pairs")
        _, info = _run(e, w, "the same again")
        assert info["attempts"] == 1 and info["pairs_cap"] == 4 * cc.PAIRS_CAP0
    finally:
        e.close()


def test_more_tuples_than_the_scratch_of_a_block_starts_with(tmp_path):
    pairs_ladder_body(tmp_path)


# ------------------------------------------------------------------------------------------------ g. the capacity of the global table
EXT_MESSAGE = "more than 49152 references share seeds with one read"


def ext_capacity_body(tmp_path, mode=0):
    """49 152 members are accepted (oracle records), 49 153 are SMR_ERR_CAPACITY with the documented message, and the context goes on working.
    (chain_build_set counts a member when it takes its slot and reports the overflow at the first count above 3/4 of the slots; its probe loop
    makes at most `slots` steps, so a full table ends it.)"""
    ok = cc.ext_limit_workload(str(tmp_path), cc.EXT_SET_MEMBERS)
    over = cc.ext_limit_workload(str(tmp_path), cc.EXT_SET_MEMBERS + 1)
    for w, m in ((ok, cc.EXT_SET_MEMBERS), (over, cc.EXT_SET_MEMBERS + 1)):
        x = _numbers(w, 18)[0]
        assert x["members_lo"] == x["members_hi"] == m and x["nh"] == 12 and len(w.seqs) <= 4, x
    e = _engine(mode)
    try:
        routes, info = _run(e, ok, "49 152 members", stride=18)
        assert info["retries"]["SCAP"] == 1 and info["retries"]["PAIRS"] >= 1 and info["chain_ext"] and info["pairs_cap"] >= 2 * cc.EXT_SET_MEMBERS, info
        assert all(r == cc.ROUTE_CHAIN | cc.ROUTE_EXT for r in routes)
        with pytest.raises(smr.SmrError) as err:
            over.gpu_records(e, is_reverse=0, skiplengths=[18, 18, 18])
        assert EXT_MESSAGE in str(err.value) and "rc=-4" in str(err.value), str(err.value)
        _run(e, ok, "49 152 members after the refusal", stride=18)
        w = _ordinary(tmp_path)
        _run(e, w, "an ordinary batch after the refusal")
    finally:
        e.close()


def test_49152_members_are_accepted_and_49153_refused(tmp_path):
    ext_capacity_body(tmp_path)


# ------------------------------------------------------------------------------------------------ h. more alignments than slots
SLOTS_MESSAGE = "a read produced more alignments than max_alignments_per_read"


def slots_body(tmp_path, mode=0):
    w = cc.slots_workload(str(tmp_path))
    x = _numbers(w, 18)[0]
    assert x["ncand"] == 40 and x["max_pairs"] >= 8, x
    e = _engine(mode)
    try:
        with pytest.raises(smr.SmrError) as err:
            w.gpu_records(e, num_alignments=0)                        # "all alignments" with the 32 slots smr.align gives it
        assert SLOTS_MESSAGE in str(err.value) and "rc=-4" in str(err.value), str(err.value)
        _run(e, w, "all alignments, 64 slots", num_alignments=0, max_alignments_per_read=64)     # nothing of the refused call is left
        _run(e, w, "best alignment")
    finally:
        e.close()


def test_more_alignments_than_slots_is_refused_and_leaves_nothing_behind(tmp_path):
    slots_body(tmp_path)


# ------------------------------------------------------------------------------------------------ i. everything in one batch, default strides, both strands
def mixed_batch_body(tmp_path, mode=0):
    w = cc.mixed_workload(str(tmp_path))
    # from the host's numbers: the first launch (forward strand, stride 18) sees a whole block of k_cand whose records outgrow its slice ...
    n18 = _numbers(w, 18)
    blk = n18[:cc.CAND_BLOCK]
    assert all(t == "block" for t in w.tags[:cc.CAND_BLOCK]) and all(x["ncand"] >= 1 and x["nh"] <= cc.CAND_HITS and x["npos"] == cc.MIXED_BLOCK_NPOS for x in blk), \
        collections.Counter((x["ncand"], x["nh"], x["npos"]) for x in blk)
    assert 3 * cc.MIXED_BLOCK_NPOS * cc.CAND_BLOCK > cc.CAND_BLOCK * cc.CAND_REC_WORDS
    # ... and the other kinds are there (the reads of the other strand excepted: the host's numbers are forward ones)
    n6 = _numbers(w, 6)
    kinds = collections.Counter(w.tags[i] for i, x in enumerate(n6) if x["ncand"] >= 1)
    assert kinds["tandem"] >= 3 and kinds["swapped"] >= 3 and kinds["periodic"] >= 3, kinds
    assert sum(1 for i, x in enumerate(n6) if w.tags[i] == "periodic" and x["lis_len"] < 2 <= x["lis_len_nonstrict"] and x["first_window_pairs"] > cc.WAVE_LIS_MAX) >= 3
    by18 = collections.Counter(x["npos"] for x in n18 if x["ncand"])
    assert all(by18[t] >= 1 for t in cc.POSITION_VALUES), sorted(by18.items())
    e = _engine(mode)
    try:
        _run(e, w, "mixed batch")
        _run(e, w, "mixed batch, all alignments", num_alignments=0, max_alignments_per_read=64)
    finally:
        e.close()


@MODES
def test_all_kinds_in_one_batch_with_the_default_passes(tmp_path, mode):
    mixed_batch_body(tmp_path, mode)
