"""smr_state_import / smr_counters_import: the stored per-read records (what smr_result_record hands out, Read::toBinString bytes) put back
into a batch, so that a run stopped after any (index, part) is continued by another context -- the reference does the same through its
key-value store (Read::load_db, read.cpp:467-539; processor.cpp:116-126).

1. a run split at every part boundary between two contexts gives the reference's own records (tests/golden/) and the counters of an unsplit run;
2. import -> fetch -> record is the identity, with and without CIGARs;
3. a FINISHED run (is_last_index_part = 1, aligned reads stored as done) resumed on a further DB gives the oracle's records, the done reads keep
   every byte, and the forward Smith-Waterman count of the second half is the oracle's (the done reads were really skipped);
4. the parser at its boundaries on crafted records; 5. every refusal of include/smr_hip.h, after which the context imports a good set.

Every equality is byte equality of every read's record.  test_emu_state_import.py runs the same bodies on the emulator."""
import atexit
import shutil
import struct
import tempfile

import numpy as np
import pytest

import sortmerna_amd as smr
from helpers import golden, orc, refrun
from helpers.cases import build_case

pytestmark = pytest.mark.gpu

MODES = pytest.mark.parametrize("mode", [0, 1], ids=["pg", "dfs"])
SPLIT_CASES = ["syn_multipart", "two_db_default", "two_db_all"]

_cases = {}


def case_setup(case):
    """the golden case built once per process: dict(idx, seqs, reads, steps = [(index_num, part, Index)], params per --ref, slots)"""
    if case not in _cases:
        d = tempfile.mkdtemp(prefix="smr_import_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        g = golden.load()[case]
        idx, seqs = build_case(case, d)
        params = {k: v for k, v in g["params"].items() if k not in ("max_mb", "evalue", "lnwin")}
        plist = [smr.default_params(minimal_score=x["minimal_score"], **params) for x in idx]
        steps = [(k, part, ix) for k, x in enumerate(idx) for part, ix in enumerate(x["parts"])]
        _cases[case] = dict(idx=idx, seqs=seqs, reads=smr.Reads.from_seqs(seqs), steps=steps, plist=plist, params=params,
                            slots=256 if plist[0].num_alignments == 0 else plist[0].num_alignments, golden=g)
    return _cases[case]


def n_steps(case):
    """(index, part) pairs of the case (golden.json: index parts per --ref as the reference's indexer made them)"""
    return golden.load()[case]["index_parts"] * len(golden.load()[case]["readstats"]["reads_matched_per_db"])


def run_steps(e, cs, steps, last_flags, with_cigar=True):
    for (k, part, ix), last in zip(steps, last_flags):
        p = cs["plist"][k]
        p.index_num, p.part, p.is_last_index_part = k, part, int(last)
        e.upload_index(ix, 0)
        e.align_part(0, p)
        if with_cigar:
            e.traceback(0, p)
        e.unload_index(0)


def same_records(got, exp, what):
    assert len(got) == len(exp), "%s: %d records against %d" % (what, len(got), len(exp))
    bad = [i for i, (a, b) in enumerate(zip(got, exp)) if a != b]
    assert not bad, "%s: %d records differ, first %d\n got=%s\n exp=%s" % (what, len(bad), bad[0], refrun.parse_record(got[bad[0]]), refrun.parse_record(exp[bad[0]]))


def engine(mode=0):
    e = smr.Engine(0)
    e.set_seed_mode(mode)
    return e


_unsplit = {}


def unsplit_counters(case, mode):
    if (case, mode) not in _unsplit:
        cs = case_setup(case)
        e = engine(mode)
        try:
            e.upload_reads(cs["reads"], cs["slots"])
            run_steps(e, cs, cs["steps"], [i == len(cs["steps"]) - 1 for i in range(len(cs["steps"]))])
            e.fetch()
            same_records(e.records(), golden.records(case), "%s unsplit" % case)
            _unsplit[(case, mode)] = e.counters(len(cs["idx"]))
        finally:
            e.close()
    return _unsplit[(case, mode)]


# ------------------------------------------------------------------------------------------------ 1. split runs
def split_body(case, k, mode):
    cs = case_setup(case)
    steps, n_db = cs["steps"], len(cs["idx"])
    assert 0 < k < len(steps) == n_steps(case)
    a = engine(mode)
    try:
        a.upload_reads(cs["reads"], cs["slots"])
        run_steps(a, cs, steps[:k], [False] * k)
        a.fetch()
        recs, ctr = a.records(), a.counters(n_db)
    finally:
        a.close()
    assert any(recs)
    b = engine(mode)
    try:
        b.upload_reads(cs["reads"], cs["slots"])
        b.import_state(recs)
        b.import_counters(ctr, n_db)
        run_steps(b, cs, steps[k:], [i == len(steps) - 1 for i in range(k, len(steps))])
        b.fetch()
        same_records(b.records(), golden.records(case), "%s split at %d" % (case, k))
        got = b.counters(n_db)
    finally:
        b.close()
    g = cs["golden"]
    print("%s split at %d: counters %s" % (case, k, got))
    assert got == unsplit_counters(case, mode)
    assert got["num_aligned"] == g["readstats"]["num_aligned"] and got["reads_matched_per_db"] == g["readstats"]["reads_matched_per_db"]


SPLITS = [(c, k) for c in SPLIT_CASES for k in range(1, n_steps(c))]


@MODES
@pytest.mark.parametrize("case,k", SPLITS, ids=["%s@%d" % ck for ck in SPLITS])
def test_a_split_run_equals_the_unsplit_run_and_the_reference_records(case, k, mode):
    split_body(case, k, mode)


# ------------------------------------------------------------------------------------------------ 2. round trip
def round_trip(e, reads, slots, recs, what):
    e.upload_reads(reads, slots)
    e.import_state(recs)
    e.fetch()
    same_records(e.records(), recs, what)


def round_trip_body(mode=0):
    cs = case_setup("two_db_all")
    recs = golden.records("two_db_all")
    parsed = [refrun.parse_record(r) for r in recs if r]
    assert max(len(p["alignv"]) for p in parsed) > 1 and all(len(a["cigar"]) for p in parsed for a in p["alignv"])
    e = engine(mode)
    try:
        round_trip(e, cs["reads"], cs["slots"], recs, "golden records of two_db_all")
        # records taken before any smr_traceback: no CIGARs, and none appear
        e.upload_reads(cs["reads"], cs["slots"])
        run_steps(e, cs, cs["steps"], [False, True], with_cigar=False)
        e.fetch()
        bare = e.records()
    finally:
        e.close()
    parsed = [refrun.parse_record(r) for r in bare if r]
    assert parsed and all(not a["cigar"] for p in parsed for a in p["alignv"])
    e = engine(mode)
    try:
        round_trip(e, cs["reads"], cs["slots"], bare, "records without CIGARs")
    finally:
        e.close()


def test_import_then_fetch_is_the_identity():
    round_trip_body()


# ------------------------------------------------------------------------------------------------ 3. a finished run, resumed on a further DB
def resume_finished(mode=0, case="two_db_default"):
    """-> (records of the first context, records of the second, oracle records after DB 1, after DB 2, SW counts engine / oracle of the second half)"""
    cs = case_setup(case)
    first = [s for s in cs["steps"] if s[0] == 0]
    second = [s for s in cs["steps"] if s[0] == 1]
    # the oracle driven the same way: DB 1 to its end as if it were the last, then DB 2
    run = orc.Run(cs["seqs"])
    oparams = {k: v for k, v in cs["golden"]["params"].items() if k not in ("max_mb", "evalue")}
    sw = []
    orecs = []
    for k, x in enumerate(cs["idx"]):
        p = orc.default_params(minimal_score=x["minimal_score"], index_num=k, **oparams)
        for part in range(x["stats"].nparts):
            p.part, p.is_last_index_part = part, int(part == x["stats"].nparts - 1)
            run.align_part(x["prefix"], x["db"], x["stats"], part, p)
        sw.append(run.counters.n_sw_fwd)
        orecs.append(run.records())
    run.close()
    a = engine(mode)
    try:
        a.upload_reads(cs["reads"], cs["slots"])
        run_steps(a, cs, first, [i == len(first) - 1 for i in range(len(first))])
        a.fetch()
        recs_a, ctr = a.records(), a.counters(2)
    finally:
        a.close()
    b = engine(mode)
    try:
        b.upload_reads(cs["reads"], cs["slots"])
        b.import_state(recs_a)
        b.import_counters(ctr, 2)
        b.prof_reset()
        run_steps(b, cs, second, [i == len(second) - 1 for i in range(len(second))])
        b.fetch()
        recs_b, sw_b = b.records(), b.prof().n_sw_fwd
    finally:
        b.close()
    return recs_a, recs_b, orecs[0], orecs[1], sw_b, sw[1] - sw[0]


def resume_finished_body(mode=0):
    recs_a, recs_b, o1, o2, sw_b, sw_o = resume_finished(mode)
    same_records(recs_a, o1, "DB 1 to its end")
    same_records(recs_b, o2, "resumed on DB 2")
    done = [i for i, r in enumerate(recs_a) if r and r[24]]
    assert done
    assert all(recs_b[i] == recs_a[i] for i in done), "a read stored as done changed"
    print("resumed on DB 2: %d reads stored as done, forward Smith-Waterman calls engine %d, oracle %d" % (len(done), sw_b, sw_o))
    assert sw_b == sw_o


@MODES
def test_a_finished_run_resumes_on_a_further_db_like_the_oracle(mode):
    resume_finished_body(mode)


# ------------------------------------------------------------------------------------------------ 4. the parser at its boundaries
def make_record(readlen, cigars, num_alignments=1, seed=0, idcov=(0, 0, 0, 0), lie=None):
    """Read::toBinString bytes with made-up field values: one alignment per entry of `cigars` (each a list of u32 words).  lie = dict of
    deliberate inconsistencies for the refusals (n_align, asz_delta, last_rl_delta)"""
    lie = lie or {}
    rng = np.random.Generator(np.random.PCG64(seed))
    r32 = lambda: int(rng.integers(0, 2 ** 31))      # noqa: E731
    body = b""
    for q, cg in enumerate(cigars):
        rl = 8 + 4 * len(cg) + 24 + 6 + 1
        cl = len(cg)
        if q == len(cigars) - 1 and "last_rl_delta" in lie:
            rl += 4 * lie["last_rl_delta"]
            cl += lie["last_rl_delta"]
        body += struct.pack("<QQ", rl % 2 ** 64, cl % 2 ** 64) + struct.pack("<%dI" % len(cg), *cg)
        body += struct.pack("<IiiiiI", r32(), r32(), r32(), r32() % readlen, r32() % readlen, readlen) + struct.pack("<HHHB", r32() & 0xFFFF, r32() % 7, r32() % 3, q & 1)
    tail = struct.pack("<II", r32(), r32()) + struct.pack("<Q", lie.get("n_align", len(cigars))) + body
    head = struct.pack("<II4I", r32() % 3, r32() % 7, *idcov) + struct.pack("<BBB", q_done(seed), 1, 0) + struct.pack("<H", r32() & 0xFFFF) + struct.pack("<iI", num_alignments, r32())
    return head + struct.pack("<Q", len(tail) + lie.get("asz_delta", 0)) + tail


def q_done(seed):
    return seed & 1


def crafted_batch(n=200, slots=4, seed=7):
    rng = np.random.Generator(np.random.PCG64(seed))
    seqs = ["".join("ACGT"[c] for c in rng.integers(0, 4, int(rng.integers(30, 140)))) for _ in range(n)]
    cig = lambda w, s: [int(x) for x in np.random.Generator(np.random.PCG64(s)).integers(1, 2 ** 32, w)]      # noqa: E731
    recs = []
    for i, s in enumerate(seqs):
        na = 1 + i % slots                              # 1 .. slots alignments: read 3 (and every fourth) has exactly `slots`
        words = [[1, 70, 0, 130][(i + q) % 4] if i % 5 else 1 + (i + q) % 3 for q in range(na)]       # CIGARs of 0, 1, 2, 3, 70 and 130 words: the lanes wrap
        recs.append(make_record(len(s), [cig(w, 1000 * i + q) for q, w in enumerate(words)], num_alignments=slots, seed=i))
    return seqs, recs


def boundaries_body():
    slots = 4
    seqs, full = crafted_batch(slots=slots)
    reads = smr.Reads.from_seqs(seqs)
    n = len(seqs)
    assert n <= 256
    lens = [len(refrun.parse_record(r)["alignv"]) for r in full]
    cl = {len(a["cigar"]) for r in full for a in refrun.parse_record(r)["alignv"]}
    assert max(lens) == slots and {1, 70, 130} <= cl and max(cl) > 64
    starts = np.cumsum([0] + [len(r) for r in full])[:-1]
    assert {int(s) % 4 for s in starts} == {0, 1, 2, 3}
    sets = {"first and last only": [full[i] if i in (0, n - 1) else b"" for i in range(n)],
            "no record at all": [b""] * n,
            "every read": full,
            "every third read": [full[i] if i % 3 == 0 else b"" for i in range(n)]}
    e = engine()
    try:
        for what, recs in sets.items():
            round_trip(e, reads, slots, recs, what)
        # into a batch that already holds results: the whole stored state is replaced
        e.import_state(sets["first and last only"])
        e.fetch()
        same_records(e.records(), sets["first and last only"], "a second import over the first")
    finally:
        e.close()
        reads.free()


def test_the_parser_at_its_boundaries():
    boundaries_body()


# ------------------------------------------------------------------------------------------------ 5. refusals
ARG, CAPACITY, STATE = "rc=-1", "rc=-4", "rc=-5"


def refusals_body():
    slots = 4
    seqs, good = crafted_batch(slots=slots)
    reads = smr.Reads.from_seqs(seqs)
    n = len(seqs)
    j = n - 1                                              # the last record: anything read past it is past the buffer
    cg = [[16, 33], [48]]
    L = len(seqs[j])

    def with_last(rec):
        return good[:j] + [rec]

    bad = [
        ("a record cut one byte short", with_last(good[j][:-1]), ARG, "do not add up"),
        ("one extra trailing byte", with_last(good[j] + b"\0"), ARG, "do not add up"),
        ("a record cut inside its header", with_last(good[j][:40]), ARG, "do not add up"),
        ("an alignment's length overshoots the record", with_last(make_record(L, cg, slots, lie=dict(last_rl_delta=1))), ARG, "do not add up"),
        ("a CIGAR length of 2^62", with_last(make_record(L, cg, slots, lie=dict(last_rl_delta=2 ** 62 - 1))), ARG, "do not add up"),
        ("alignment_size off by four", with_last(make_record(L, cg, slots, lie=dict(asz_delta=4))), ARG, "do not add up"),
        ("n_align larger than the alignments that follow", with_last(make_record(L, cg, slots, lie=dict(n_align=3))), ARG, "do not add up"),
        ("n_align = slots + 1", with_last(make_record(L, [[16]] * (slots + 1), slots)), CAPACITY, "more alignments than max_alignments_per_read"),
        ("a wrong readlen", with_last(make_record(L + 1, cg, slots)), ARG, "readlen"),
        ("a non-zero %coverage word", with_last(make_record(L, cg, slots, idcov=(0, 0, 1, 0))), ARG, "smr_idcov_part is not supported"),
        ("records with differing num_alignments", with_last(make_record(L, cg, slots + 1)), ARG, "num_alignments"),
        ("n different from the batch size", good[:j], ARG, "for a batch of"),
    ]
    e = engine()
    try:
        for what, recs, code, word in bad:
            e.upload_reads(reads, slots)
            with pytest.raises(smr.SmrError) as err:
                e.import_state(recs)
            assert code in str(err.value) and word in str(err.value), (what, str(err.value))
            e.fetch()
            assert not any(e.records()), what              # the batch is as the upload left it
            e.import_state(good)                           # ... and the context goes on working
            e.fetch()
            same_records(e.records(), good, "the good set after: " + what)
        # a refusal over a batch that held results leaves nothing of them either
        with pytest.raises(smr.SmrError):
            e.import_state(bad[0][1])
        e.fetch()
        assert not any(e.records())
    finally:
        e.close()
        reads.free()


def test_refusals_leave_a_fresh_batch_and_a_usable_context():
    refusals_body()


def after_idcov_body():
    cs = case_setup("two_db_default")
    recs = golden.records("two_db_default")
    e = engine()
    try:
        e.upload_reads(cs["reads"], cs["slots"])
        e.import_state(recs)
        k, part, ix = cs["steps"][0]
        p = cs["plist"][k]
        p.index_num, p.part = k, part
        e.upload_index(ix, 0)
        e.idcov_part(0, p, 0.97, 0.97)                     # counts the imported alignments of DB 1 (they carry their CIGARs)
        assert sum(e.idcov_counters().values()) > 0
        for call in (lambda: e.import_state(recs), lambda: e.import_counters([0, 0, 0, 0], 2)):
            with pytest.raises(smr.SmrError) as err:
                call()
            assert STATE in str(err.value) and "smr_idcov_part" in str(err.value), str(err.value)
        e.reset_state()
        e.import_state(recs)
        e.fetch()
        same_records(e.records(), recs, "after smr_state_reset")
    finally:
        e.close()


def test_import_after_the_id_coverage_pass_is_a_state_error():
    after_idcov_body()
