"""The bodies of test_gpu_cand_limits.py on the emulator (the kernel sources compiled for the host, tests/emu): the candidate stage at its
path boundaries and capacity limits, without a GPU.  Same bodies, another library behind the binding.

Time budget of the default run: about two minutes on 8 cores (the CPU suite has one).  By default every case runs once -- the position counts at both
strides with the default paths and once with SMR_WALK_GATHER=0, the slice overflow with and without gather, the LIS variants, the LDS -> global switch,
the PAIRS ladder, the refused slots --; SMR_EMU_FULL=1 adds both seed kernels, SMR_HANDOVER=0, the capacity of the global table (a DB of
49 153 references: the slowest case) and the mixed batch."""
import os

import pytest

from helpers import emu
from test_gpu_cand_limits import (position_counts_body, hit_counts_body, slice_overflow_body, lis_variant_body, lds_to_ext_body, pairs_ladder_body,
                                  ext_capacity_body, slots_body, mixed_batch_body, POSITION_VARIANTS)

FULL = os.environ.get("SMR_EMU_FULL", "0") == "1"
_MODES = [0, 1] if FULL else [0]
_ids = lambda v: ",".join("%s=%s" % kv for kv in v.items()) or "default" if isinstance(v, dict) else None      # noqa: E731


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


_POS = [(s, e, m) for s in (18, 3) for e in POSITION_VARIANTS for m in _MODES] if FULL else [(18, POSITION_VARIANTS[0], 0), (3, POSITION_VARIANTS[0], 0), (18, POSITION_VARIANTS[1], 0)]


@pytest.mark.parametrize("stride,env,mode", _POS, ids=lambda v: _ids(v) if isinstance(v, dict) else str(v))
def test_reads_with_63_to_257_positions_take_the_way_the_host_model_says(tmp_path, monkeypatch, stride, env, mode):
    position_counts_body(tmp_path, monkeypatch, stride, env, mode)


def test_reads_with_64_and_65_seed_hits(tmp_path):
    hit_counts_body(tmp_path)


@pytest.mark.parametrize("mode", _MODES, ids=lambda m: "dfs" if m else "pg")
@pytest.mark.parametrize("gather", [1, 0], ids=["gather", "gather0"])
def test_a_block_whose_records_outgrow_its_slice(tmp_path, monkeypatch, gather, mode):
    slice_overflow_body(tmp_path, monkeypatch, gather, mode)


def test_windows_of_64_and_of_65_to_80_pairs(tmp_path):
    lis_variant_body(tmp_path)


def test_a_set_of_384_members_and_one_of_385(tmp_path):
    lds_to_ext_body(tmp_path)


def test_more_tuples_than_the_scratch_of_a_block_starts_with(tmp_path):
    pairs_ladder_body(tmp_path)


@pytest.mark.skipif(not FULL, reason="SMR_EMU_FULL=1 (a DB of 49 153 references and five attempts over 98 000 positions)")
def test_49152_members_are_accepted_and_49153_refused(tmp_path):
    ext_capacity_body(tmp_path)


def test_more_alignments_than_slots_is_refused_and_leaves_nothing_behind(tmp_path):
    slots_body(tmp_path)


@pytest.mark.skipif(not FULL, reason="SMR_EMU_FULL=1")
def test_all_kinds_in_one_batch_with_the_default_passes(tmp_path):
    mixed_batch_body(tmp_path, 0)
