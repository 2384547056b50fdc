"""The library's environment switches (csrc/smr_tuning.hpp): a context reads every one of them once, in smr_create, and Engine.tuning()
(smr_tuning_text) hands out what it latched.  On the emulator (tests/emu), with SMR_SW_SELFCHECK=0 so that creating a context costs nothing.
Every expected value below is written out from the expression that read the variable before there was a table (the getenv calls that stood in
smr_engine.hip, smr_engine_seed.hpp and smr_engine_trace.hpp): defaults, clamps, and what atoi makes of a string that is no number (0, which the
clamp then treats like any other 0)."""
import os
import re

import pytest

import sortmerna_amd as smr
from helpers import emu, paths

# (the self-check's default is SMR_SW_SELFCHECK_CASES: 512 on the device, 8 in the emulator's shim; every context here is created with it set to 0)
DEFAULTS = {
    "SMR_SW_PACKED": 2, "SMR_SEED_EXACT": 0, "SMR_SEED_SHARED": 1, "SMR_SEED_DEDUP": 1024, "SMR_SEED_HOT_BIN": 262144, "SMR_SEED_HOT_SUB": 65536,
    "SMR_SEG_INLINE": 1, "SMR_HANDOVER": 1, "SMR_WALK_SPLIT": 1, "SMR_WALK_ROUNDS": 8, "SMR_WALK_K": 4, "SMR_WALK_GATHER": 1, "SMR_WALK_ASSUME": 3,
    "SMR_BEGINS_X4": 0, "SMR_PG_HOST": 0, "SMR_TRACE_GLOBAL_ROWS": 0, "SMR_CAND_BLOOM": 128, "SMR_PG_CAND_CAP": 256, "SMR_SEED_POOL_WORDS": 0,
    "SMR_CIGAR_POOL_WORDS": 0, "SMR_SW_SELFCHECK": 0, "SMR_VERBOSE": 0, "SMR_SEED_DEBUG": 0, "SMR_WALK_DEBUG": 0, "SMR_DEBUG_PHASES": 0,
}
RETIRED = ["SMR_PG_GRID", "SMR_PG_SWZ", "SMR_PG_LDS_PAD", "SMR_TRACE_BPC", "SMR_CHAIN_WPC"]

# name -> [(value in the environment, value the context holds)]: each bound, one step outside it, a string that is no number
CASES = {
    "SMR_WALK_ROUNDS": [("1", 1), ("32", 32), ("0", 1), ("33", 32), ("x", 1), ("-5", 1)],                          # max(1, min(32, atoi))
    "SMR_WALK_K": [("1", 1), ("15", 15), ("0", 1), ("16", 15), ("x", 1)],                                           # max(1, min(WK_MAX = 15, atoi))
    "SMR_CAND_BLOOM": [("64", 64), ("512", 512), ("63", 64), ("513", 512), ("x", 64), ("65", 128), ("129", 256), ("128", 128)],      # next power of two, 64..512
    "SMR_PG_CAND_CAP": [("4", 4), ("2048", 2048), ("3", 4), ("2049", 2048), ("x", 4), ("8", 8)],                    # min(2048, max(4, atoi))
    "SMR_SEED_POOL_WORDS": [("64", 64), ("0x7FFFFFF0", 0x7FFFFFF0), ("63", 64), ("0x7FFFFFF1", 0x7FFFFFF0), ("x", 64), ("0200", 128), ("0x100", 256)],   # strtoull base 0, C_NSHARD = 64 .. 0x7FFFFFF0
    "SMR_CIGAR_POOL_WORDS": [("16", 16), ("17", 17), ("15", 16), ("4294967296", 1 << 32), ("x", 16), ("0x40", 16)],  # strtoull base 10, at least 16
    "SMR_SEED_DEDUP": [("0", 0), ("1", 1), ("-1", 0), ("2", 2), ("x", 0)],                                          # max(0, atoi)
    "SMR_SEED_HOT_BIN": [("1", 1), ("2", 2), ("0", 1), ("64", 64), ("x", 1), ("-3", 1)],                            # max(1, atoi)
    "SMR_SEED_HOT_SUB": [("1", 1), ("2", 2), ("0", 1), ("200", 200), ("x", 1), ("-3", 1)],                          # max(1, atoi)
    "SMR_SEG_INLINE": [("0", 0), ("1", 1), ("-1", 1), ("2", 1), ("x", 0)],                                          # off only for the value 0 (which "x" is to atoi)
    "SMR_SEED_EXACT": [("0", 0), ("1", 1), ("2", 1), ("x", 0)],                                                     # atoi != 0
    "SMR_PG_HOST": [("0", 0), ("1", 1), ("2", 1), ("x", 0)],                                                        # atoi != 0
    "SMR_SW_PACKED": [("0", 0), ("1", 1), ("2", 2), ("x", 0)],                                                      # atoi
    "SMR_SEED_SHARED": [("0", 0), ("2", 2), ("1", 1), ("x", 0)],
    "SMR_HANDOVER": [("0", 0), ("1", 1), ("x", 0)],
    "SMR_WALK_SPLIT": [("0", 0), ("1", 1), ("x", 0)],
    "SMR_WALK_GATHER": [("0", 0), ("1", 1), ("x", 0)],
    "SMR_WALK_ASSUME": [("0", 0), ("100", 100), ("x", 0)],                                                          # (uint32_t)atoi
    "SMR_SW_SELFCHECK": [("0", 0), ("x", 0)],
    # set = on, whatever the value
    "SMR_BEGINS_X4": [("1", 1), ("0", 1), ("x", 1)],
    "SMR_TRACE_GLOBAL_ROWS": [("1", 1), ("0", 1), ("x", 1)],
    "SMR_SEED_DEBUG": [("1", 1), ("0", 1)],
    "SMR_WALK_DEBUG": [("1", 1), ("0", 1)],
    "SMR_DEBUG_PHASES": [("1", 1), ("0", 1)],
    "SMR_VERBOSE": [("1", 1), ("0", 1)],
}


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in list(DEFAULTS) + RETIRED:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("SMR_SW_SELFCHECK", "0")


def _tuning():
    e = smr.Engine(0)
    try:
        return e.tuning()
    finally:
        e.close()


def _differences(got, exp):
    return {k: (got.get(k), exp.get(k)) for k in set(got) | set(exp) if got.get(k) != exp.get(k)}


def test_a_clean_environment_gives_the_defaults():
    assert not _differences(_tuning(), DEFAULTS)


def test_every_switch_has_cases():
    assert set(CASES) == set(DEFAULTS)


@pytest.mark.parametrize("k", range(max(len(v) for v in CASES.values())))
def test_clamps_at_their_bounds_outside_them_and_on_strings_that_are_no_numbers(monkeypatch, k):
    """the k-th case of every switch that has one, all in one context"""
    exp = dict(DEFAULTS)
    for name, cases in CASES.items():
        if k < len(cases):
            monkeypatch.setenv(name, cases[k][0])
            exp[name] = cases[k][1]
    assert not _differences(_tuning(), exp), "(got, expected) with %s" % {n: c[k][0] for n, c in CASES.items() if k < len(c)}


def test_retired_names_are_absent_and_change_nothing(monkeypatch):
    for name, v in zip(RETIRED, ("1", "1", "4096", "1", "1")):
        monkeypatch.setenv(name, v)
    got = _tuning()
    assert not set(RETIRED) & set(got)
    assert not _differences(got, DEFAULTS)


def test_a_context_keeps_what_it_read_when_it_was_created(monkeypatch):
    first = {name: cases[0] for name, cases in CASES.items()}
    for name, (v, _) in first.items():
        monkeypatch.setenv(name, v)
    exp = {name: x for name, (_, x) in first.items()}
    e = smr.Engine(0)
    try:
        assert not _differences(e.tuning(), exp)
        for name in list(DEFAULTS) + RETIRED:                 # deleted one by one, then all gone
            monkeypatch.delenv(name, raising=False)
            assert not _differences(e.tuning(), exp), name
        for name in list(DEFAULTS) + RETIRED:                 # set one by one to something else, then all set
            monkeypatch.setenv(name, "7")
            assert not _differences(e.tuning(), exp), name
    finally:
        e.close()
    # ... and a context created now reads what is there now
    for name in DEFAULTS:
        monkeypatch.delenv(name)
    monkeypatch.setenv("SMR_SW_SELFCHECK", "0")
    assert not _differences(_tuning(), DEFAULTS)


def _documented():
    """{name: default as written} of the table of a context's switches in INTEGRATION.md"""
    rows, inside = {}, False
    for line in open(os.path.join(paths.REPO, "INTEGRATION.md")):
        if line.startswith("| Switch of a context |"):
            inside = True
        elif inside and not line.startswith("|"):
            break
        elif inside:
            m = re.match(r"\| `(SMR_[A-Z0-9_]+)` \| ([^|]*) \|", line)
            if m:
                rows[m.group(1)] = m.group(2).strip()
    return rows


def test_the_documented_table_names_the_same_switches_with_the_same_defaults():
    doc = _documented()
    assert set(doc) == set(_tuning())
    assert doc.pop("SMR_SW_SELFCHECK") == "512"               # the device's SMR_SW_SELFCHECK_CASES (the emulator's shim has 8)
    assert not _differences({k: int(v) for k, v in doc.items()}, {k: v for k, v in DEFAULTS.items() if k != "SMR_SW_SELFCHECK"})
    text = open(os.path.join(paths.REPO, "INTEGRATION.md")).read()
    assert not [n for n in RETIRED if n in text]
