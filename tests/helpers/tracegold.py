"""tests/golden/trace_pairs.json.gz: (read, reference window) pairs with the alignment (score, begin/end) and the CIGAR that the
reference's own ssw_align / banded_sw returned for them (written by tests/golden/make_golden_trace.py).  TEST INFRASTRUCTURE."""
import gzip
import json
import os

import numpy as np

from . import paths

_TR = bytes.maketrans(b"ACGTN", bytes(range(5)))


def load():
    with gzip.open(os.path.join(paths.REPO, "tests", "golden", "trace_pairs.json.gz"), "rb") as f:
        g = json.loads(f.read().decode())
    return g["cases"]


def cigar_text(c):
    return "".join("%d%s" % (int(x) >> 4, "MID"[int(x) & 15]) for x in c)


def spans(c, k=None):
    """the aligned spans of a stored case's first k pairs, cut out by ssw.c's begin / end positions: (reads, refs, scores)"""
    reads, refs, scores = [], [], []
    for rd, rf, e in zip(c["reads"][:k], c["refs"][:k], c["expected"][:k]):
        reads.append(rd.encode().translate(_TR)[e[3]:e[4] + 1])
        refs.append(rf.encode().translate(_TR)[e[1]:e[2] + 1])
        scores.append(e[0])
    return reads, refs, scores


def compare(engine, sc, reads, refs, scores, cigars, labels, whole_window=True):
    """one smr_cigar_batch call over the spans under scoring sc; every CIGAR has to equal banded_sw's.  whole_window=False: for fixtures that hold
    pairs whose walk reaches read row 0 before reference column 0 -- banded_sw stops there (ssw.c:680), and its CIGAR covers less than the window"""
    got = engine.cigar_batch(reads, refs, scores, match=sc["match"], mismatch=sc["mismatch"], score_N=sc["score_N"], gap_open=sc["gap_open"], gap_ext=sc["gap_ext"])
    assert len(got) == len(cigars)
    for i in range(len(cigars)):
        exp = np.array(cigars[i], dtype=np.uint32)
        assert got[i].tolist() == exp.tolist(), "scoring %s, %s (read span %d, reference span %d, score %d): got %s, banded_sw %s" % (
            sc, labels[i], len(reads[i]), len(refs[i]), scores[i], cigar_text(got[i]), cigar_text(exp))
        # a CIGAR consumes exactly both spans
        in_ref = sum(int(x) >> 4 for x in exp if int(x) & 15 in (0, 2))
        assert sum(int(x) >> 4 for x in exp if int(x) & 15 in (0, 1)) == len(reads[i]) and (in_ref == len(refs[i]) or not whole_window and in_ref < len(refs[i]))
    return len(cigars)


def check(engine, kinds=None, max_pairs=None, schemes=None):
    """the traceback kernels through smr_cigar_batch against banded_sw's CIGARs; returns the number of pairs checked"""
    n = 0
    for ci, c in enumerate(load()):
        if kinds is not None and c["kind"] not in kinds:
            continue
        if schemes is not None and ci // 4 not in schemes:
            continue
        k = len(c["reads"]) if max_pairs is None else min(max_pairs, len(c["reads"]))
        reads, refs, scores = spans(c, k)
        n += compare(engine, c["scoring"], reads, refs, scores, c["cigars"][:k], ["%s pair %d" % (c["kind"], i) for i in range(k)])
    return n


def check_variants():
    """the same vectors through the code paths that ordinary inputs do not reach: DP rows of the wide kernel in global memory (bands too
    wide for LDS) and a CIGAR pool that has to be regrown several times.  A context reads its switches when it is created: one context per
    variant, made after the variant's variables are set and closed before the next"""
    import sortmerna_amd as smr
    variants = [({"SMR_TRACE_GLOBAL_ROWS": "1"}, [dict(kinds=["indels"], max_pairs=40), dict(kinds=["long"], max_pairs=2, schemes=[0, 2])]),
                ({"SMR_CIGAR_POOL_WORDS": "64"}, [dict(kinds=["short", "indels"], max_pairs=60, schemes=[0])])]
    names = [k for env, _ in variants for k in env]
    n = 0
    try:
        for env, runs in variants:
            for k in names:
                os.environ.pop(k, None)
            os.environ.update(env)
            engine = smr.Engine(0)
            try:
                for kw in runs:
                    n += check(engine, **kw)
            finally:
                engine.close()
    finally:
        for k in names:
            os.environ.pop(k, None)
    return n
