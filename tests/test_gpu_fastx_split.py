"""smr_fastx_split: the aligned.* / other.* FASTX streams of a batch whose text stayed on the device (SMR_FASTX_KEEP), sized, routed and
serialised by kernels (csrc/smr_fxsplit.hpp).

The yardstick of every test is the host model of helpers/fxsplit.py -- the host parser's record_text and a restatement of the writer's routing,
pinned to the writer itself by test_fxsplit_model.py --, never the code under test.  Every comparison is for equality.  The texts are those of
test_gpu_fastx_device.py: they sit on the parser's edges and on this kernel's too (records that start at every byte phase of the output,
trimmed bytes, wrapped FASTA, CRLF, a missing final newline, counts around a wave and a block of the scans, a header and a record longer
than a team of lanes copies).  test_emu_fastx_split.py runs the same bodies on the kernel emulator."""
import ctypes as C
import os
import random

import pytest

import sortmerna_amd as smr
from sortmerna_amd import capi
from helpers import golden
from helpers.fxsplit import VALID_OPTS, expected_streams, opts_id
from test_gpu_fastx_device import DRESSINGS, IRREGULAR, SCAN_COUNTS, boundary_text, case_run, dress, is_regular, long_text, scan_text

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CAPACITY, ERR_STATE = -1, -4, -5
NAMES = ["aligned[%d]" % j for j in range(4)] + ["other[%d]" % j for j in range(4)]


def host_reads(data, tmp_path, name="reads.txt"):
    path = os.path.join(str(tmp_path), name)
    with open(path, "wb") as f:
        f.write(data)
    return smr.Reads.from_fastx_text(path)


def upload_keep(e, data, tmp_path, batch=None, name="reads.txt", device_path=True):
    """data into the selected batch (or batch `batch`) with its text kept -> the host parser's Reads of the same bytes"""
    want = host_reads(data, tmp_path, name)
    e.upload_fastx(data, 1, batch=batch, view=True, keep=True).free()
    info = e.fastx_info()
    assert info[0] == (0 if device_path else 1) and info[2] == want.count, info
    return want


def split_equals_model(e, reads, hits, what, **opts):
    got = e.fastx_split(hit=hits, **{k: v for k, v in opts.items() if k != "reads"})
    want = expected_streams(reads, hits, opts)
    for k in range(8):
        assert got[k] == want[k], "%s: %s (%d bytes, %d expected)" % (what, NAMES[k], len(got[k]), len(want[k]))
    return got


def hit_patterns(n, seed):
    rng = random.Random(seed)
    return {"none": [0] * n, "all": [1] * n, "alternating from 0": [(i + 1) & 1 for i in range(n)], "alternating from 1": [i & 1 for i in range(n)],
            "only the first": [int(i == 0) for i in range(n)], "only the last": [int(i == n - 1) for i in range(n)], "random": [rng.randrange(2) for _ in range(n)]}


# ------------------------------------------------------------------------------------------------ 1. boundaries
def boundaries_body(fastq, how, tmp_path):
    e = smr.Engine(0)
    try:
        data = dress(boundary_text(fastq), how)
        reads = upload_keep(e, data, tmp_path)
        try:
            starts = set()
            sizes = [_record_len(reads, i) for i in range(reads.count)]
            for name, hits in hit_patterns(reads.count, 20261018).items():
                got = split_equals_model(e, reads, hits, "%s, %s, hits %s" % ("fastq" if fastq else "fasta", how, name))
                assert sum(len(s) for s in got) == sum(sizes)               # the same records, wherever they go
                at = [0, len(got[0])]                                       # where aligned[0] and other[0] begin in the output
                for i in range(reads.count):
                    k = 0 if hits[i] else 1
                    starts.add(at[k] & 3)
                    at[k] += sizes[i]
            assert starts == {0, 1, 2, 3}, starts
        finally:
            reads.free()
    finally:
        e.close()


def _record_len(reads, i):
    h, s, q = reads.record_text(i)
    return len(h.encode()) + 1 + len(s.encode()) + 1 + ((2 + len(q.encode()) + 1) if reads.is_fastq else 0)


@pytest.mark.parametrize("how", DRESSINGS)
@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_boundaries(fastq, how, tmp_path):
    boundaries_body(fastq, how, tmp_path)


# ------------------------------------------------------------------------------------------------ 2. scans
def scan_body(fastq, n_rec, tmp_path):
    e = smr.Engine(0)
    try:
        reads = upload_keep(e, scan_text(fastq, n_rec), tmp_path)
        try:
            rng = random.Random(n_rec)
            for name, hits in [("random", [rng.randrange(2) for _ in range(n_rec)]), ("runs of 64", [(i // 64) & 1 for i in range(n_rec)]),
                               ("runs of 65", [1 - ((i // 65) & 1) for i in range(n_rec)])]:
                got = split_equals_model(e, reads, hits, "%d records, hits in %s" % (n_rec, name))
                assert [k for k in range(8) if got[k]] in ([0, 4], [0], [4]), "a stream that does not exist is not empty"
            if n_rec % 2 == 0:
                hits = [rng.randrange(2) for _ in range(n_rec)]
                split_equals_model(e, reads, hits, "%d records, interleaved" % n_rec, layout=1)
                split_equals_model(e, reads, hits, "%d records, interleaved, four files" % n_rec, layout=1, out2=True, sout=True)
        finally:
            reads.free()
        if fastq and n_rec == max(SCAN_COUNTS):                                 # pairs across the blocks of all eight scans
            reads = upload_keep(e, scan_text(fastq, n_rec + 1), tmp_path)
            try:
                rng = random.Random(1)
                split_equals_model(e, reads, [rng.randrange(2) for _ in range(n_rec + 1)], "%d records, interleaved, four files" % (n_rec + 1), layout=1, out2=True, sout=True)
            finally:
                reads.free()
    finally:
        e.close()


@pytest.mark.parametrize("n_rec", SCAN_COUNTS)
@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_scans(fastq, n_rec, tmp_path):
    scan_body(fastq, n_rec, tmp_path)


# ------------------------------------------------------------------------------------------------ 3. a long header, a long record
def long_body(fastq, tmp_path):
    e = smr.Engine(0)
    try:
        reads = upload_keep(e, long_text(fastq), tmp_path)
        try:
            n = reads.count
            for i in ([1] if fastq else [1, 2]):                                # the long header (FASTQ: and the 5 000 letters); the wrapped record
                split_equals_model(e, reads, [int(k == i) for k in range(n)], "record %d is the hit" % i)
                split_equals_model(e, reads, [int(k != i) for k in range(n)], "record %d is the only miss" % i)
        finally:
            reads.free()
    finally:
        e.close()


@pytest.mark.parametrize("fastq", [True, False], ids=["fastq", "fasta"])
def test_a_header_and_a_record_longer_than_a_team_copies(fastq, tmp_path):
    long_body(fastq, tmp_path)


# ------------------------------------------------------------------------------------------------ 4. pairs
def pairs_text():
    """64 pairs of FASTQ, headers of varied length -> the records, mate 1 and mate 2 alternating"""
    rng = random.Random(64)
    recs = []
    for k in range(64):
        for m in (1, 2):
            n = 1 + rng.randrange(70)
            seq = bytes(rng.choice(b"ACGTN") for _ in range(n))
            recs.append(b"@p%d%s/%d\n%s\n+\n%s\n" % (k, b"x" * (k % 11), m, seq, bytes(33 + rng.randrange(40) for _ in range(n))))
    return recs


def pairs_body(tmp_path):
    e = smr.Engine(0)
    try:
        recs = pairs_text()
        rng = random.Random(4)
        pair_hits = [(k & 1, (k >> 1) & 1) for k in range(64)]                  # all four patterns of a pair, 16 times each
        rng.shuffle(pair_hits)
        inter = [h for p in pair_hits for h in p]
        # layout 1: the interleaved text in the selected batch
        e.select_batch(0)
        reads = upload_keep(e, b"".join(recs), tmp_path)
        try:
            for o in VALID_OPTS:
                for al, ot in [(True, True), (True, False), (False, True)]:
                    split_equals_model(e, reads, inter, "interleaved, %s, aligned=%s other=%s" % (opts_id(o), al, ot), layout=1, aligned=al, other=ot, **o)
        finally:
            reads.free()
        # layout 2: the same mates in two batches
        r1 = upload_keep(e, b"".join(recs[0::2]), tmp_path, name="mates1.fq")
        r2 = upload_keep(e, b"".join(recs[1::2]), tmp_path, batch=1, name="mates2.fq")
        try:
            hits = inter[0::2] + inter[1::2]
            for o in VALID_OPTS:
                for al, ot in [(True, True), (True, False), (False, True)]:
                    what = "two batches, %s, aligned=%s other=%s" % (opts_id(o), al, ot)
                    got = e.fastx_split(layout=2, mates=1, hit=hits, aligned=al, other=ot, **o)
                    want = expected_streams((r1, r2), hits, dict(layout=2, aligned=al, other=ot, **o))
                    for k in range(8):
                        assert got[k] == want[k], "%s: %s" % (what, NAMES[k])
        finally:
            r1.free()
            r2.free()
    finally:
        e.close()


def test_pairs_under_every_option_set(tmp_path):
    pairs_body(tmp_path)


# ------------------------------------------------------------------------------------------------ 5. irregular text
def irregular_body(tmp_path):
    e, e2 = smr.Engine(0), smr.Engine(0)                                        # e2 never holds kept text
    try:
        for what, data in IRREGULAR.items():
            try:
                want = host_reads(data, tmp_path)
            except smr.SmrError:
                with pytest.raises(smr.SmrError):
                    e2.upload_fastx(data, keep=True)
                with pytest.raises(smr.SmrError) as x:
                    e2.fastx_split()
                assert "rc=%d" % ERR_STATE in str(x.value) and "SMR_FASTX_KEEP" in str(x.value), what
                continue
            try:
                e.upload_fastx(data, keep=True).free()
                assert e.fastx_info()[0] == (0 if is_regular(data) else 1), what
                rng = random.Random(len(data))
                for _ in range(3):
                    split_equals_model(e, want, [rng.randrange(2) for _ in range(want.count)], what)
            finally:
                want.free()
    finally:
        e.close()
        e2.close()


def test_irregular_text_with_keep(tmp_path):
    irregular_body(tmp_path)


# ------------------------------------------------------------------------------------------------ 6. the batch's own hits
OWN_HITS_CASES = ["t9", "real_default"]


def own_hits_body(case, tmp_path):
    e = smr.Engine(0)
    try:
        kept = {}

        def up(path, slots):
            kept["reads"] = smr.Reads.from_fastx_text(path)
            e.upload_fastx(path, slots, view=True, keep=True).free()
            assert e.fastx_info()[0] == 0
            n = kept["reads"].count
            assert e.fastx_split() == expected_streams(kept["reads"], [0] * n, {}), "before any alignment every read is in other[0]"

        recs, _, is_hit = case_run(e, case, tmp_path, up)
        try:
            assert recs == golden.records(case), "keeping the text changed the records"
            assert any(is_hit) and (case == "t9" or not all(is_hit)), "the case shows nothing"          # (t9 is one read)
            assert e.fastx_split() == expected_streams(kept["reads"], is_hit, {})
            assert e.fastx_split(other=False) == expected_streams(kept["reads"], is_hit, dict(other=False))
        finally:
            kept["reads"].free()
    finally:
        e.close()


@pytest.mark.parametrize("case", OWN_HITS_CASES)
def test_the_batchs_own_hits(case, tmp_path):
    own_hits_body(case, tmp_path)


# ------------------------------------------------------------------------------------------------ 7. guards
def guards_body(tmp_path):
    e = smr.Engine(0)
    L = e.L
    try:
        data = scan_text(True, 65)
        off, need = (C.c_uint64 * 9)(), C.c_uint64()

        def split(layout=0, mates=-1, buf=None, cap=0, **kw):
            o = capi.FxSplitOpts(layout, kw.get("paired_in", 0), kw.get("paired_out", 0), 0, 0, 1, 1)
            return L.smr_fastx_split(e.h, mates, C.byref(o), None, buf, cap, off, C.byref(need))

        def usable():
            got = e.fastx_split(hit=hits)
            assert got == want, "the context is not usable after a refusal"

        # no kept text
        e.upload_fastx(data).free()
        assert split() == ERR_STATE and b"SMR_FASTX_KEEP" in L.smr_last_error(e.h)
        reads = upload_keep(e, data, tmp_path)
        hits = [i % 3 == 0 for i in range(reads.count)]
        want = expected_streams(reads, hits, {})
        usable()
        # another upload into the batch drops the text; a state reset keeps it
        assert L.smr_reads_upload(e.h, reads.h, 1) == 0
        assert split() == ERR_STATE and b"SMR_FASTX_KEEP" in L.smr_last_error(e.h)
        upload_keep(e, data, tmp_path).free()
        e.reset_state()
        usable()
        # capacity: one byte short, then 64 bytes to spare
        assert split() == 0
        total = need.value
        unaligned = expected_streams(reads, [0] * reads.count, {})[4]               # (own hits: nothing has been aligned)
        assert total == len(unaligned) == sum(len(s) for s in want) and list(off) == [0, 0, 0, 0, 0, total, total, total, total]
        buf = (C.c_uint8 * (total + 64))(*([0xA5] * (total + 64)))
        need.value = 0
        assert split(buf=buf, cap=total - 1) == ERR_CAPACITY
        assert need.value == total and off[4] == 0 and off[5] == total and off[8] == total and bytes(buf) == b"\xa5" * (total + 64)
        usable()
        assert split(buf=buf, cap=total + 64) == 0
        assert bytes(buf)[:total] == unaligned and bytes(buf)[total:] == b"\xa5" * 64
        # layouts 1 and 2
        assert split(layout=1) == ERR_ARG                                       # 65 reads
        usable()
        assert split(layout=2, mates=0) == ERR_ARG                              # the selected batch
        usable()
        upload_keep(e, scan_text(True, 64), tmp_path, batch=1).free()
        assert split(layout=2, mates=1) == ERR_ARG                              # 65 reads, 64 mates
        usable()
        upload_keep(e, scan_text(True, 64), tmp_path).free()
        assert split(layout=1, paired_in=1, paired_out=1) == ERR_ARG and split(layout=2, mates=1, paired_in=1, paired_out=1) == ERR_ARG
        assert split(layout=3) == ERR_ARG and L.smr_fastx_split(e.h, -1, None, None, None, 0, off, C.byref(need)) == ERR_ARG
        upload_keep(e, scan_text(False, 64), tmp_path, batch=1).free()
        assert split(layout=2, mates=1) == ERR_ARG                              # FASTQ reads, FASTA mates
        reads.free()
        reads = upload_keep(e, data, tmp_path)
        usable()
        assert e.fastx_split(hit=hits) == e.fastx_split(hit=hits) == want        # a second identical call
        reads.free()
    finally:
        e.close()


def test_guards(tmp_path):
    guards_body(tmp_path)
