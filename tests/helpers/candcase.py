"""Crafted workloads for the candidate stage (k_cand -> k_wlist -> k_walk / k_wnext, k_chain<EXT = false | true>) and a host-side model of the way a
read takes through it.  TEST INFRASTRUCTURE ONLY.

The model uses nothing of the library under test: the numbers of a read come from the oracle's unit entry points (orc_window_hits,
orc_index_positions), and the constants that decide the route are restated below as literals -- if one of them changes in the kernels, the
tests that use this file have to be told."""
import ctypes as C
import os
from collections import Counter

import numpy as np

import sortmerna_amd as smr

from . import orc
from .workload import Workload, iseq_for_strand, GUMBEL_UNIFORM

# smr_chain.hpp / smr_walk.hpp / smr_engine.hip, restated (not imported)
LNWIN = 18
CAND_HITS = 64            # seed hits of a read k_cand scans; more: the read is marked without a position count
CAND_REC_MAX = 64         # positions of a record
CAND_BLOCK = 256          # reads per block of k_cand; its records share CAND_BLOCK * CAND_REC_WORDS words
CAND_REC_WORDS = 32
CAND_GROUP = 16           # reads of a block that place their records at the same time (their order among themselves is not defined)
WK_MAX_POS = 128          # positions of a read k_walk gathers itself
WK_MAX_ROWS = 256         # longest read of the walk rounds
WAVE_LIS_MAX = 64         # pairs of one window wave_lis_first takes; more: serial_lis_first
LDS_SET_MEMBERS = 384     # members the LDS table of a wave holds (3/4 of chain_scap = 512 slots)
EXT_SET_MEMBERS = 49152   # members the global table of a block holds (3/4 of CH_EXT_CAP = 65 536 slots)
PAIRS_CAP0 = 4096         # tuples per block before the first C_ERR_PAIRS
ROUTE_RECORD, ROUTE_GATHER, ROUTE_CHAIN, ROUTE_EXT = 1, 2, 4, 8

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


# ------------------------------------------------------------------------------------------------
# the host's numbers of a read
# ------------------------------------------------------------------------------------------------
class HostIndex:
    """part 0 of a workload's index as the oracle loads it"""

    def __init__(self, wl):
        self.L = orc.lib()
        self.ix = self.L.orc_index_load(wl.prefix.encode(), 0, LNWIN)
        assert self.ix, "index load failed"
        self._ids = (C.c_uint32 * 8192)()
        self._pos = {}

    def close(self):
        if self.ix:
            self.L.orc_index_free(self.ix)
            self.ix = None

    def positions(self, id_):
        got = self._pos.get(id_)
        if got is None:
            n = self.L.orc_index_positions(self.ix, id_, None, 0)
            buf = np.zeros((max(n, 1), 2), dtype=np.uint32)
            self.L.orc_index_positions(self.ix, id_, buf.ctypes.data, n)
            got = self._pos[id_] = buf[:n]                   # (reference position, reference number)
        return got

    def numbers(self, seq, stride, num_seeds=2):
        """forward strand, one pass of `stride`: dict(len, nh, npos, hit_seeds, ncand, max_pairs, first_window_pairs, members_lo, members_hi, lis_strict)"""
        out = dict(len=len(seq), nh=0, npos=0, hit_seeds=0, ncand=0, max_pairs=0, first_window_pairs=0, members_lo=0, members_hi=0, lis_strict=False, lis_len=0, lis_len_nonstrict=0)
        if len(seq) < LNWIN:
            return out
        v = iseq_for_strand(seq, 0)
        z = C.c_int()
        per_ref = Counter()
        pairs = {}
        for k in range((len(seq) - LNWIN + stride) // stride):
            n = self.L.orc_window_hits(self.ix, v.ctypes.data, k * stride, LNWIN, 0, 0, self._ids, 8192, C.byref(z))
            assert n <= 8192
            out["nh"] += n
            out["hit_seeds"] += 1 if n else 0
            for q in range(n):
                pa = self.positions(self._ids[q])
                out["npos"] += len(pa)
                if len(pa) <= 4096:                          # (the pairs themselves only where a test looks at them: short lists)
                    for p, s in pa:
                        pairs.setdefault(int(s), []).append((int(p), k * stride))
                per_ref.update(Counter(pa[:, 1].tolist()))
        out["members_hi"] = len(per_ref)
        out["members_lo"] = sum(1 for c in per_ref.values() if c >= 2)
        cand = [s for s, c in per_ref.items() if c >= num_seeds]
        out["ncand"] = len(cand)
        out["max_pairs"] = max((per_ref[s] for s in cand), default=0)
        # the first window of read length over the best candidate's pairs (alignment.cpp:203-241): everything up to begin_ref + len - begin_read - lnwin + 1
        if cand:
            best = min(cand, key=lambda s: (-per_ref[s], s))
            pr = sorted(pairs.get(best, []))
            if pr:
                end = pr[0][0] + len(seq) - pr[0][1] - LNWIN + 1
                win = [q for p, q in pr if p <= end]
                out["first_window_pairs"] = len(win)
                out["lis_strict"] = _lis_len(win) < len(win)
                out["lis_len"], out["lis_len_nonstrict"] = _lis_len(win), _lis_len(win, strict=False)
        return out


def _lis_len(a, strict=True):
    import bisect
    tails = []
    for x in a:
        i = bisect.bisect_left(tails, x) if strict else bisect.bisect_right(tails, x)
        if i == len(tails):
            tails.append(x)
        else:
            tails[i] = x
    return len(tails)


def _record_fate(i, want, cur, room, nums):
    """does read i of a group get a record?  True / False, or None where it depends on the order in which the group's reads take their room"""
    if i not in want:
        return False
    if cur + sum(3 * nums[j]["npos"] for j in want) <= room:
        return True                                          # the whole group fits
    if cur + 3 * min(nums[j]["npos"] for j in want) > room:
        return False                                         # not even the smallest record of the group fits
    return None


def expected_routes(nums, marked, num_seeds=2, gather=True, handover=True, ext=False):
    """The route byte of every read of a single-launch run (one strand, one pass) from the host's numbers; None where the kernels leave it open.
    marked[i]: the device marked read i (k_cand's Bloom filter may mark reads without a candidate; they take room in their block's slice like the others).
    ext: the context has switched to the global tables (after a C_ERR_SCAP)."""
    n = len(nums)
    out = [0] * n
    room = CAND_BLOCK * CAND_REC_WORDS
    for b0 in range(0, n, CAND_BLOCK):
        eligible = [i for i in range(b0, min(n, b0 + CAND_BLOCK)) if nums[i]["hit_seeds"] >= num_seeds and nums[i]["nh"] > 0]
        cur = 0                                              # words of the block's slice given out so far
        for g0 in range(0, len(eligible), CAND_GROUP):
            grp = eligible[g0:g0 + CAND_GROUP]
            want = [i for i in grp if handover and marked[i] and num_seeds >= 2 and nums[i]["nh"] <= CAND_HITS and 0 < nums[i]["npos"] <= CAND_REC_MAX]
            for i in grp:
                if not marked[i]:
                    continue
                x = nums[i]
                has_record = _record_fate(i, want, cur, room, nums)
                in_rounds = handover and x["len"] <= WK_MAX_ROWS             # the walk rounds take the read at all
                scanned = num_seeds >= 2 and x["nh"] <= CAND_HITS            # k_cand counted its positions
                if has_record is None:
                    out[i] = None
                elif has_record and in_rounds:
                    out[i] = ROUTE_RECORD
                elif not has_record and in_rounds and gather and scanned and 1 <= x["npos"] <= WK_MAX_POS:
                    out[i] = ROUTE_GATHER
                elif x["members_hi"] <= LDS_SET_MEMBERS:
                    out[i] = ROUTE_CHAIN
                elif x["members_lo"] <= LDS_SET_MEMBERS:
                    out[i] = None                            # (whether the set outgrows the LDS table depends on Bloom collisions of references that occur once)
                else:
                    out[i] = (ROUTE_CHAIN | ROUTE_EXT) if ext else ROUTE_CHAIN
            cur += sum(3 * nums[i]["npos"] for i in want)
    return out


# ------------------------------------------------------------------------------------------------
# the generator
# ------------------------------------------------------------------------------------------------
class Crafted:
    """a DB of random background references and planted motifs, and reads drawn from the motifs; everything seeded"""

    def __init__(self, seed):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.refs = []
        self.reads = []
        self.tags = []

    def rand(self, n):
        return _ACGT[self.rng.integers(0, 4, n)].tobytes().decode()

    @staticmethod
    def anti(s):
        """a letter that differs from every letter of s, place by place (what follows a cut copy: no window reaches over the cut with one error)"""
        return s.translate(str.maketrans("ACGT", "CGTA"))

    def mutate(self, s, rate):
        if rate <= 0:
            return s
        a = np.frombuffer(s.encode(), dtype=np.uint8).copy()
        m = self.rng.random(len(a)) < rate
        a[m] = _ACGT[(np.searchsorted(_ACGT, a[m]) + self.rng.integers(1, 4, int(m.sum()))) % 4]
        return a.tobytes().decode()

    def background(self, n_refs, length=400):
        for _ in range(n_refs):
            self.refs.append(self.rand(length))

    def plant(self, motif, copies, cut=0, sub_rate=0.0, flank=30, first_exact=True):
        """`copies` references that hold the motif (the first one exactly, the others with substitutions at sub_rate), and -- cut > 0 -- one more
        that holds its first `cut` letters only"""
        for k in range(copies):
            body = motif if (k == 0 and first_exact) else self.mutate(motif, sub_rate)
            self.refs.append(self.rand(flank) + body + self.rand(flank))
        if cut:
            self.refs.append(self.rand(flank) + motif[:cut] + self.anti(motif[cut:cut + LNWIN]) + self.rand(flank))

    def read(self, seq, tag):
        self.reads.append(seq)
        self.tags.append(tag)
        return len(self.reads) - 1

    def positions_case(self, target, stride, windows, tag=None, sub_rate=0.0):
        """a read of `windows` windows whose motif lies in target // windows references + the first target % windows windows of it in one more:
        `target` positions when every copy is hit by every window"""
        ln = LNWIN + (windows - 1) * stride
        motif = self.rand(ln)
        full, rem = divmod(target, windows)
        self.plant(motif, full, cut=(LNWIN + (rem - 1) * stride) if rem else 0, sub_rate=sub_rate)
        return self.read(motif, tag if tag is not None else "npos%d" % target)

    def write_db(self, path, shuffle=True):
        order = np.arange(len(self.refs))
        if shuffle:
            self.rng.shuffle(order)
        with open(path, "w") as f:
            for n, k in enumerate(order):
                f.write(">r%d\n%s\n" % (n, self.refs[k]))
        return path

    def workload(self, tmpdir, name="crafted", shuffle=True):
        tmpdir = os.path.join(tmpdir, name)                 # (a Workload names its index files after its directory)
        os.makedirs(tmpdir, exist_ok=True)
        db = self.write_db(os.path.join(tmpdir, name + ".fasta"), shuffle)
        w = Workload(tmpdir, db_fasta=db, seqs=self.reads)
        w.tags = list(self.tags)
        return w


def set_reads(w, seqs, tags=None):
    """another batch of reads against the same index"""
    w.seqs = list(seqs)
    w.reads = smr.Reads.from_seqs(w.seqs)
    lam, K = GUMBEL_UNIFORM
    w.minimal_score = smr.minimal_score(lam, K, w.parts[0].info(), len(w.seqs), sum(map(len, w.seqs)))
    w.tags = list(tags) if tags is not None else [""] * len(w.seqs)
    return w


POSITION_VALUES = (63, 64, 65, 127, 128, 129, 256, 257)
# windows of a read of at most WK_MAX_ROWS letters, and at most CAND_HITS of them, per stride
_WINDOWS = {18: (7, 8, 9, 11, 13, 14), 3: (32, 43, 48, 56, 64)}


def positions_workload(tmpdir, stride, seed=71, per_value=10, background=60):
    """reads with 63 .. 257 positions at `stride` (POSITION_VALUES), per_value of each, in random order among reads without any hit"""
    c = Crafted(seed + stride)
    c.background(background)
    jobs = []
    for t in POSITION_VALUES:
        for k in range(per_value):
            jobs.append((t, _WINDOWS[stride][(k + t) % len(_WINDOWS[stride])], 0.01 if k % 5 == 4 else 0.0))
    jobs += [(0, 0, 0.0)] * 40
    for j in c.rng.permutation(len(jobs)):
        t, w, sub = jobs[j]
        if t:
            c.positions_case(t, stride, w, sub_rate=sub)
        else:
            c.read(c.rand(int(c.rng.integers(40, 200))), "background")
    return c.workload(tmpdir, "pos_s%d" % stride)


def hits_workload(tmpdir, seed=83, per_value=8):
    """stride 3, a motif that occurs once: reads of 64 and of 65 windows (207 / 210 letters) = 64 against 65 seed hits"""
    c = Crafted(seed)
    c.background(40)
    for k in range(per_value):
        for windows in (64, 65, 63):
            motif = c.rand(LNWIN + (windows - 1) * 3)
            c.plant(motif, 1)
            c.read(motif, "nh%d" % windows)
    return c.workload(tmpdir, "hits")


def slice_workload(tmpdir, seed=89, npos=17):
    """stride 3.  Block 0 (reads 0..255): every read a motif of its own with `npos` windows, one copy = npos positions and a record of 3 * npos
    words each: with 17 the first ten groups of sixteen fill 8 160 of the slice's 8 192 words and no later read of the block finds room, whatever the order inside
    a group.  Block 1 (reads 256..): 100 of the same reads, which all find room in their own slice."""
    c = Crafted(seed)
    c.background(20)
    for k in range(CAND_BLOCK + 100):
        motif = c.rand(LNWIN + (npos - 1) * 3)
        c.plant(motif, 1, flank=10)
        c.read(motif, "block%d" % (k // CAND_BLOCK))
    return c.workload(tmpdir, "slice")


def lis_workload(tmpdir, seed=97):
    """stride 6, reads U U of a reference that holds U U (U: 100..125 random letters) = every window at two places of ONE reference, one period apart: a first
    window of 65..80 pairs whose longest increasing run is a strict subsequence; next to them reads of one copy with exactly 64 pairs (stride 3, 64 windows)"""
    c = Crafted(seed)
    c.background(40)
    for k in range(12):
        u = c.rand(100 + 2 * k)
        windows = 34 + (k % 6)
        ln = LNWIN + (windows - 1) * 6
        c.refs.append(c.rand(30) + (u + u + u)[:max(ln, 2 * len(u))] + c.rand(30))
        c.read((u + u + u)[:ln], "tandem")
    for k in range(8):
        # a rearranged reference: the two halves of the read's motif in swapped order (its pairs come out of order along the reference)
        motif = c.rand(LNWIN + 39 * 6)
        h = len(motif) // 2
        c.refs.append(c.rand(30) + motif[h:] + motif[:h] + c.rand(30))
        c.read(motif, "swapped")
    periodic_reads(c)
    return c.workload(tmpdir, "lis")


PERIOD3 = ("ACG", "ACT", "AGT", "CGT", "AGC", "ATC", "ATG", "CTG")      # the eight period-3 words of three different letters (up to rotation)


def periodic_reads(c, read_len=250):
    """Reads whose first window is six periods of a three-letter word and whose second window lies in ANOTHER reference; a reference holds 66..78
    periods' worth of that window, three letters apart.  The candidate's pairs then all have read position 0: more than 64 of them in the first
    window of read length, and the longest STRICTLY increasing run (find_lis, alignment.cpp:58-98) is one pair -- below min_lis = 2, no
    Smith-Waterman call -- while a run that took equal read positions would hold them all."""
    for k, word in enumerate(PERIOD3):
        occ = 66 + (k * 5) % 13                              # occurrences of the window: 66..78
        other = c.rand(LNWIN)
        c.refs.append(c.rand(30) + word * (6 + occ - 1) + c.anti(word * 6) + c.rand(30))
        c.refs.append(c.rand(40) + other + c.rand(40))
        c.read(word * 6 + other + c.rand(read_len - 2 * LNWIN), "periodic")


def family_workload(tmpdir, members, seed=101, n_reads=6, copy_len=60, sub_rate=0.005, name=None):
    """`members` references of copy_len letters around one motif (near-identical copies): a read of the motif shares at least two seeds with each"""
    c = Crafted(seed + members)
    c.background(30)
    motif = c.rand(copy_len)
    # (the copies differ behind their last window only -- the letters from 54 on at stride 18 --, so every copy keeps all its seeds: the member count is exact)
    keep = LNWIN * ((copy_len - LNWIN) // LNWIN + 1)
    for k in range(members):
        c.refs.append(c.rand(12) + motif[:keep] + (motif[keep:] if k == 0 else c.mutate(motif[keep:], 40 * sub_rate)) + c.rand(12))
    for k in range(n_reads):
        c.read(motif if k % 2 == 0 else c.mutate(motif, 0.02), "family%d" % members)
    for k in range(6):
        c.read(c.refs[k][20:170], "ordinary")
    return c.workload(tmpdir, name or "family%d" % members)


def pairs_workload(tmpdir, seed=103, copies=350, windows=14):
    """stride 18: reads of 14 windows whose motif lies in 350 references (0.5 % substitutions) = some 4 500 tuples, more than the 4 096 a block starts with, in a set of 350 members
    (the LDS table holds them: no C_ERR_SCAP mixes in)"""
    c = Crafted(seed)
    c.background(30)
    motif = c.rand(LNWIN + (windows - 1) * 18)
    c.plant(motif, copies, sub_rate=0.005, flank=10)
    for k in range(3):
        c.read(motif if k == 0 else c.mutate(motif, 0.01), "pairs")
    for k in range(6):
        c.read(c.refs[k][30:180], "ordinary")
    return c.workload(tmpdir, "pairs")


def ext_limit_workload(tmpdir, members, seed=107, groups=6, n_reads=2):
    """A read of 2 * groups seeds S0 S1 ... (12 x 18 = 216 letters) and a DB in which ONE reference holds the whole read and members - 1 references of 60 letters hold
    one pair of neighbouring seeds each (group g: S2g, 20 random letters, S2g+1, 4 random letters; at most 8 192 per seed, below the 10 000 positions an index list keeps):
    `members` references occur at least twice among the read's positions, the full one first in the candidate order (twelve seeds)."""
    c = Crafted(seed)
    seeds = [c.rand(LNWIN) for _ in range(2 * groups)]
    read = "".join(seeds)
    c.refs.append(c.rand(20) + read + c.rand(20))
    short = members - 1
    per = [short // groups + (1 if g < short % groups else 0) for g in range(groups)]
    assert max(per) <= 9000
    filler = _ACGT[c.rng.integers(0, 4, (short, 24))]
    k = 0
    for g in range(groups):
        for _ in range(per[g]):
            c.refs.append(seeds[2 * g] + filler[k, :20].tobytes().decode() + seeds[2 * g + 1] + filler[k, 20:].tobytes().decode())      # (the index keeps no seed that ends a reference)
            k += 1
    for _ in range(n_reads):
        c.read(read, "ext%d" % members)
    return c.workload(tmpdir, "ext%d" % members, shuffle=False)


def slots_workload(tmpdir, seed=109, copies=40):
    """a motif in 40 references, exact copies: with "all alignments" a read of it aligns to 40 references"""
    c = Crafted(seed)
    c.background(30)
    motif = c.rand(150)
    c.plant(motif, copies)
    c.read(motif, "slots")
    for k in range(6):
        c.read(c.refs[k][30:180], "ordinary")
    return c.workload(tmpdir, "slots")


MIXED_BLOCK_NPOS = 12     # positions of a read of mixed_workload's first block at stride 18: 4 windows x 3 references


def mixed_workload(tmpdir, seed=113):
    """All kinds in one batch, for runs with the default strides on both strands.  Reads 0..255 = one block of k_cand: 256 forward reads of four
    windows at stride 18 whose motif lies in three references = 12 positions and a record of 36 words each, 9 216 words for a slice of 8 192 in
    the first launch.  Then position reads (63..257 at stride 18 and at stride 3), 63 / 64 / 65-hit reads, tandem, swapped and periodic reads, a
    third of them from the other strand."""
    c = Crafted(seed)
    c.background(60)
    for k in range(CAND_BLOCK):
        motif = c.rand(LNWIN + 3 * 18)
        c.plant(motif, 3, flank=10)
        c.read(motif, "block")
    for k in range(3):
        for t in POSITION_VALUES:
            c.positions_case(t, 18, _WINDOWS[18][(k + t) % 6], sub_rate=0.01 if k == 2 else 0.0)
            c.positions_case(t, 3, _WINDOWS[3][(k + t) % 5])
    for windows in (63, 64, 65):
        motif = c.rand(LNWIN + (windows - 1) * 3)
        c.plant(motif, 1)
        c.read(motif, "nh%d" % windows)
    for k in range(6):
        u = c.rand(100 + 4 * k)
        ln = LNWIN + (34 + k) * 6
        c.refs.append(c.rand(30) + (u + u + u)[:max(ln, 2 * len(u))] + c.rand(30))
        c.read((u + u + u)[:ln], "tandem")
    for k in range(6):
        motif = c.rand(LNWIN + 39 * 6)
        h = len(motif) // 2
        c.refs.append(c.rand(30) + motif[h:] + motif[:h] + c.rand(30))
        c.read(motif, "swapped")
    periodic_reads(c)
    comp = str.maketrans("ACGT", "TGCA")
    c.reads = [s if (k < CAND_BLOCK or k % 3) else s.translate(comp)[::-1] for k, s in enumerate(c.reads)]      # a third of the others from the other strand
    return c.workload(tmpdir, "mixed")
