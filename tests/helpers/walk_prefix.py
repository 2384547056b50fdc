"""The candidate walk with prefix tasks (smr_walk.hpp: a look-ahead task of a read that is expected to align is scored over the first
SMR_WALK_PREFIX per cent of its window; the interval decides it or the task is scored again in full): records byte-equal to the oracle's on
a family workload under every mode, tasks-per-read and option set, and -- from smr_walk_prefix_stats -- the new path really taken where it
applies and never where the options rule it out.  Shared by tests/test_gpu_walk_prefix.py and tests/test_emu_walk_prefix.py.
TEST INFRASTRUCTURE."""
import sortmerna_amd as smr
from .workload import Workload

# SMR_WALK_PREFIX: off; every window four columns (nearly everything undecided: the path that scores a task again); about 40 % of a window;
# every prefix as long as its window (no prefix task at all)
MODES = {"off": 0, "cols4": 1, "cols40pct": 44, "whole": 100}
WALK_K = (1, 4, 15)
OPTIONS = {"best1": {}, "best3": {"num_alignments": 3}, "two_not_best": {"is_best": 0, "num_alignments": 2}, "all": {"num_alignments": 0}}
ELIGIBLE = ("best1", "best3")          # P.is_best && P.num_alignments > 0


def workload(tmpdir, n_reads):
    return Workload(str(tmpdir), db_nt=300_000, n_reads=n_reads, frac_db=0.4, seed=5, family_size=40)


class Oracle:
    """the oracle's records per option set, computed once"""

    def __init__(self, w):
        self.w, self.got = w, {}

    def __call__(self, opt):
        if opt not in self.got:
            self.got[opt] = self.w.oracle_records(**OPTIONS[opt])
        return self.got[opt]


def backed_off(st):
    """adapt_walk_prefix's rule on the counts of ONE part: off after a part that consumed at least 64 intervals, fewer than two decided per undecided one"""
    return st["decided"] + st["redone"] >= 64 and st["decided"] < 2 * st["redone"]


def run_case(w, oracle, monkeypatch, mode, k, opt, rounds=None):
    """-> the prefix statistics of the run, after the records, the hit count and the number of ssw_align calls were found equal to the oracle's.
    SMR_WALK_K = 1 is the LEAST a read leaves per round (walk_tasks_per_read): round 0 then has no look-ahead and later rounds may or may not, so
    those cases check the records alone and could pass without a prefix task; the counts are asserted for k > 1.
    rounds = 2 (SMR_WALK_ROUNDS): round 0 leaves the tasks, the closing round k_walk<true> is the only one that consumes results -- every
    undecided interval counted then was scored again INSIDE that kernel."""
    monkeypatch.setenv("SMR_WALK_PREFIX", str(MODES[mode]))
    if rounds is not None:
        monkeypatch.setenv("SMR_WALK_ROUNDS", str(rounds))
    monkeypatch.setenv("SMR_WALK_K", str(k))
    monkeypatch.setenv("SMR_SW_SELFCHECK", "0")
    exp, ctr = oracle(opt)
    e = smr.Engine(0)
    try:
        got, c = w.gpu_records(e, **OPTIONS[opt])
        st = e.walk_prefix_stats()
        what = "SMR_WALK_PREFIX=%d SMR_WALK_K=%d %s" % (MODES[mode], k, opt)
        assert st["percent"] == MODES[mode], (what, st)
        assert st["live"] == (0 if backed_off(st) else 1), (what, st)      # (one part: the context's decision after it)
        assert got == exp, "%s: %d records differ (prefix tasks %s)" % (what, sum(1 for a, b in zip(got, exp) if a != b), st)
        assert c["num_aligned"] == ctr["num_aligned"], what
        assert e.prof().n_sw_fwd == ctr["n_sw_fwd"], (what, e.prof().n_sw_fwd, ctr["n_sw_fwd"], st)
    finally:
        e.close()
    assert st["scored"] == st["decided"] + st["redone"] + st["unused"], (what, st)
    if opt not in ELIGIBLE:
        assert st["scored"] == 0 and st["ahead"] == 0, (what, st)
    if mode in ("off", "whole"):
        assert st["scored"] == 0, (what, st)
    # (SMR_WALK_K = 1 is the least a read leaves: round 0 has no look-ahead then, later rounds with few listed reads may -- nothing is asked of the counts)
    if opt in ELIGIBLE and k > 1:
        assert st["ahead"] > 0 and st["ahead_cells"] >= st["ahead"], (what, st)      # (the census is taken whatever the mode)
        if mode in ("cols4", "cols40pct"):
            assert st["scored"] > 0, (what, st)
    if opt == "best1" and k > 1 and mode == "cols40pct":
        assert st["decided"] > 0, (what, st)
    if opt == "best1" and k > 1 and mode == "cols4":
        assert st["redone"] > 0, (what, st)
    return st


def check_back_off(w, oracle, monkeypatch):
    """prefixes of four columns decide next to nothing: after the first part the context leaves no prefix task, the second run over the same
    reads scores none, and its records are the oracle's again; smr_prof_reset does not switch the mode back on"""
    monkeypatch.setenv("SMR_WALK_PREFIX", str(MODES["cols4"]))
    monkeypatch.setenv("SMR_WALK_K", "4")
    monkeypatch.setenv("SMR_SW_SELFCHECK", "0")
    exp, ctr = oracle("best1")
    e = smr.Engine(0)
    try:
        got, _ = w.gpu_records(e)
        first = e.walk_prefix_stats()
        assert got == exp and first["scored"] > 0 and backed_off(first) and first["live"] == 0, first
        got, _ = w.gpu_records(e)
        second = e.walk_prefix_stats()
        assert got == exp
        assert second["scored"] == first["scored"] and second["live"] == 0 and second["ahead"] > first["ahead"], (first, second)
        e.prof_reset()
        got, _ = w.gpu_records(e)
        third = e.walk_prefix_stats()
        assert got == exp and third["scored"] == 0 and third["live"] == 0 and third["ahead"] > 0, third
    finally:
        e.close()
