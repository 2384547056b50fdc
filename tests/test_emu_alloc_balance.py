"""Every device allocation of a context is freed by the time it is destroyed.  The engine's device arrays own themselves (smr_devbuf.hpp); this
test keeps that true: on the emulator (tests/emu), whose hipMalloc keeps a table of what is live, a context is walked through its life on a
small golden workload -- the records still the reference's -- and the table must be back where it started."""
import ctypes

import numpy as np
import pytest

import sortmerna_amd as smr
from helpers import emu, golden
from helpers.cases import build_case

CASE = "syn_multipart"           # the smallest golden workload whose index has more than one part


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        lib.emu_live_allocations.restype = ctypes.c_size_t
        lib.emu_live_allocations.argtypes = []
        yield lib


@pytest.fixture(scope="module")
def case(tmp_path_factory, emulator):
    idx, seqs = build_case(CASE, tmp_path_factory.mktemp("idx"))
    assert len(idx) == 1 and len(idx[0]["parts"]) >= 2
    yield idx[0], seqs, golden.records(CASE)
    for ix in idx[0]["parts"]:
        ix.free()


def _run_batch(e, parts, p, exp):
    """the selected batch through align, traceback, fetch, the id / coverage pass and the state export; its records against `exp`"""
    for part in range(len(parts)):
        p.part = part
        p.is_last_index_part = int(part == len(parts) - 1)
        e.align_part(part, p)
        e.traceback(part, p)
    e.fetch()
    got = e.records()
    bad = [i for i, (a, b) in enumerate(zip(got, exp)) if a != b]
    assert len(got) == len(exp) and not bad, "%d records differ from the reference's, first %s" % (len(bad), bad[:1])
    for part in range(len(parts)):
        p.part = part
        e.idcov_part(part, p, 0.97, 0.97)
    e.fetch()
    assert e.export_records() == e.records()


@pytest.mark.parametrize("env", [{}, {"SMR_SEED_POOL_WORDS": "4096", "SMR_PG_CAND_CAP": "8"}], ids=["default", "regrow"])
def test_the_allocations_of_a_context_balance(emulator, case, monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d, seqs, exp = case
    parts = d["parts"]
    live0 = emulator.emu_live_allocations()
    e = smr.Engine(0)
    assert emulator.emu_live_allocations() > live0                  # (the table is on: SMR_EMU_GUARD=0 would count nothing)
    for s, ix in enumerate(parts):
        e.upload_index(ix, s)
    reads = smr.Reads.from_seqs(seqs)
    cut = len(seqs) // 3
    tail = reads.slice(cut, len(seqs) - cut)
    p = smr.default_params(minimal_score=d["minimal_score"])
    e.select_batch(0)
    e.upload_reads(reads, 1)
    e.upload_reads_batch(1, tail, 1)
    _run_batch(e, parts, p, exp)
    e.select_batch(1)
    e.n_reads = tail.count
    _run_batch(e, parts, p, exp[cut:])
    if env:
        assert e.seed_pool_info()["grown"] >= 1 and e.prof().n_seed_redo > 0      # the retry ladder did reallocate
    # the seams that build a throw-away batch: three pairs each
    spans = [bytes(np.random.default_rng(7 + k).integers(0, 4, 40 + 25 * k, dtype=np.uint8)) for k in range(3)]
    cig = e.cigar_batch(spans, spans, [2 * len(x) for x in spans])
    assert [list(c) for c in cig] == [[len(x) << 4] for x in spans]
    out = e.idcov_batch(spans, spans, cig, [0] * 3, [len(x) - 1 for x in spans], [len(x) for x in spans], 0.97, 0.97)
    assert [tuple(r[:3]) for r in out] == [(0, 0, len(x)) for x in spans]
    # a refused call allocates nothing that stays
    live = emulator.emu_live_allocations()
    with pytest.raises(smr.SmrError, match=r"empty or oversized pair \(rc=-1\)"):             # SMR_ERR_ARG
        e.cigar_batch([spans[0], b""], [spans[0], spans[1]], [80, 0])
    assert emulator.emu_live_allocations() == live
    e.unload_index(0)
    assert emulator.emu_live_allocations() < live
    e.close()
    tail.free()
    reads.free()
    assert emulator.emu_live_allocations() == live0
