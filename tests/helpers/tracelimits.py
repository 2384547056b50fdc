"""tests/golden/trace_limits.json.gz: constructed (read, reference window) pairs that sit on the limits of the traceback kernels -- every hand-over
of the band ladder, the strip counts of the wide kernel, the outermost diagonals of a band, the 24 staged CIGAR runs -- with the alignment and
the CIGAR the reference's own ssw_align / banded_sw returned for them (written by tests/golden/make_golden_trace_limits.py), and the bodies of
tests/test_gpu_trace_limits.py / tests/test_emu_trace_limits.py over them.  TEST INFRASTRUCTURE."""
import gzip
import json
import os

from . import paths, tracegold

CLASSES = ("gap", "shift", "edge", "runs", "tiny", "fill", "big")
N_PAIRS = 608
SHORT_SPAN = 300                 # "short": both spans at most this (what the mixed and the replicated batches take)
WIDEST_GAPS = (2046, 2047)       # initial bands 2047 | 2048: the last two levels of the wide kernel, windows of about 1 100 x 3 150

_cases = None
_pairs = None


class Pair:
    """one stored pair: the spans cut out by ssw.c's positions, the CIGAR, and where its path runs"""
    def __init__(self, c, i):
        rd, rf, sc = tracegold.spans(dict(reads=[c["reads"][i]], refs=[c["refs"][i]], expected=[c["expected"][i]]))
        self.kind, self.scheme, self.scoring, self.name = c["kind"], c["scheme"], c["scoring"], c["names"][i]
        self.read, self.ref, self.score, self.cigar = rd[0], rf[0], sc[0], c["cigars"][i]
        self.band0 = abs(len(self.ref) - len(self.read)) + 1
        a = b = self.dev = 0
        for x in self.cigar:                     # largest |j - i| of the path from the main diagonal
            a += (x >> 4) if x & 15 != 2 else 0
            b += (x >> 4) if x & 15 != 1 else 0
            self.dev = max(self.dev, abs(b - a))
        self.band = self.band0                   # the band banded_sw ends with: the first of band0, 2 band0 ... that holds the path
        while self.band < self.dev:
            self.band *= 2
        self.span = max(len(self.read), len(self.ref))
        self.label = "%s %s %s" % (self.kind, self.scheme, self.name)

    def gap_letters(self):
        return int(self.name[3:-1]) if self.kind == "gap" else 0


def load():
    global _cases
    if _cases is None:
        with gzip.open(os.path.join(paths.REPO, "tests", "golden", "trace_limits.json.gz"), "rb") as f:
            _cases = json.loads(f.read().decode())["cases"]
    return _cases


def pairs(classes=CLASSES, schemes=None, max_span=None, max_band=None):
    global _pairs
    if _pairs is None:
        _pairs = [Pair(c, i) for c in load() for i in range(len(c["names"]))]
    return [p for p in _pairs if p.kind in classes and (schemes is None or p.scheme in schemes) and (max_span is None or p.span <= max_span) and
            (max_band is None or p.band <= max_band)]


def by_scheme(ps):
    out = {}
    for p in ps:
        out.setdefault(p.scheme, []).append(p)
    return sorted(out.items())


def run(engine, ps):
    """one batch (all pairs of one scheme); -> the launches of the band ladder it took"""
    assert ps and all(p.scheme == ps[0].scheme for p in ps)
    engine.prof_reset()
    tracegold.compare(engine, ps[0].scoring, [p.read for p in ps], [p.ref for p in ps], [p.score for p in ps], [p.cigar for p in ps], [p.label for p in ps],
                      whole_window=False)      # (12 tiny and 2 fill pairs under S2 stop at read row 0 short of the window's first column)
    return int(engine.prof().trace_launches)


def check(engine, classes, widest_gaps=False, **sel):
    """every stored pair of the classes, one batch per class and scheme; the gaps of WIDEST_GAPS letters only with widest_gaps, in a batch of their own
    (their flag tiles in the last level are 20 MB per block: four blocks at most); returns the number of pairs checked"""
    n = 0
    for kind in classes:
        for _, ps in by_scheme(pairs((kind,), **sel)):
            wide = [p for p in ps if p.gap_letters() in WIDEST_GAPS]
            rest = [p for p in ps if p.gap_letters() not in WIDEST_GAPS]
            if rest:
                run(engine, rest); n += len(rest)
            if wide and widest_gaps:
                assert len(wide) <= 4
                run(engine, wide); n += len(wide)
    return n


def ladder_launches(band):
    """launches until a pair that ends with this band has its CIGAR, the narrow kernels fitting: k_trace_band<8> holds bands up to 3, k_trace_band<16>
    up to 7, k_trace_wide up to 31 | 255 | 2047 level by level"""
    return 1 + sum(band > cap for cap in (3, 7, 31, 255, 2047))


def check_rungs(engine):
    """each gap / shift / edge pair that ends within band 255 alone: the number of launches tells which kernel finished it"""
    n = 0
    for p in pairs(("gap", "shift", "edge"), max_band=255):
        got = run(engine, [p])
        assert got == ladder_launches(p.band), "%s (initial band %d, path up to diagonal %d, final band %d): %d launches, the ladder has %d for it" % (
            p.label, p.band0, p.dev, p.band, got, ladder_launches(p.band))
        n += 1
    return n


def check_widest_rungs(engine, kinds="ID"):
    """the gaps of 2 046 | 2 047 letters (the narrow kernels do not fit their windows into LDS): band 2 048 takes one launch more than band 2 047 -- the
    last level, whose DP rows are in global memory without any switch"""
    n = 0
    for k in kinds:
        a, b = (next(p for p in pairs(("gap",), schemes=("S1",)) if p.name == "gap%d%s" % (d, k)) for d in WIDEST_GAPS)
        assert (a.band, b.band) == (2047, 2048)
        la, lb = run(engine, [a]), run(engine, [b])
        assert lb == la + 1, "gap of 2046 %s: %d launches, of 2047: %d" % (k, la, lb)
        n += 2
    return n


def short_pairs(scheme):
    return pairs(("gap", "shift", "edge", "runs"), schemes=(scheme,), max_span=SHORT_SPAN)


BIG_WITHOUT_NARROW = (2100, 1900)    # the batch's longest read sizes the narrow kernels' LDS (32 bytes of flags per row, 8 x 2 windows): neither fits 64 KB
BIG_WITH_NARROW = (1300,)            # ... and this one does, with 63 KB


def check_mixed(engine, big):
    """all short pairs of a scheme in one batch with the big pair of `big` letters.  Where the narrow kernels do not fit, every short alignment goes
    through k_trace_wide with a band of one strip -- one launch per level that is needed and none before; where they do, the whole ladder runs"""
    assert big in BIG_WITHOUT_NARROW + BIG_WITH_NARROW
    n = 0
    for s in ("S0", "S1", "S2"):
        ps = short_pairs(s)
        k = len(ps)
        assert k > 40 and max(p.band for p in ps) <= 255
        ps = ps[:k // 2] + [p for p in pairs(("big",), schemes=(s,)) if p.name == "big%d" % big] + ps[k // 2:]
        assert len(ps) == k + 1 and max(len(p.read) for p in ps) > big - 20
        want = ladder_launches(max(p.band for p in ps)) if big in BIG_WITH_NARROW else 1 + sum(any(p.band > cap for p in ps) for cap in (31, 255))
        got = run(engine, ps)
        assert got == want, "scheme %s with the %d-letter pair: %d launches, expected %d" % (s, big, got, want)
        n += len(ps)
    return n


def replicated(n, scheme="S1"):
    """the short pairs of a scheme over and over until there are n, every round starting one pair later: the groups of lanes of a wave get another mix every time"""
    ps = short_pairs(scheme)
    out = []
    r = 0
    while len(out) < n:
        out += ps[r % len(ps):] + ps[:r % len(ps)]
        r += 1
    return out[:n]


def grids_loop(ps, n_cu):
    """more tasks than every kernel's grid takes at once: 16 blocks per CU of 8 | 4 alignments for the narrow kernels, 32 blocks per CU of one for the wide one"""
    return len(ps) > n_cu * 16 * 8 and sum(p.band > 3 for p in ps) > n_cu * 16 * 4 and sum(p.band > 7 for p in ps) > n_cu * 32


def check_replicated(engine, n_cu, at_least=0):
    n = max(at_least, 64)
    while not grids_loop(replicated(n), n_cu):
        n += n // 2
    ps = replicated(n)
    assert run(engine, ps) == ladder_launches(max(p.band for p in ps))
    return len(ps)


def check_pool_of_16_words(engine):
    """every scheme's short pairs with a pool that one 25-run CIGAR overflows: the pool is regrown and the ladder started over, which shows as
    more launches than one pass of the ladder has"""
    n = 0
    for s in ("S0", "S1", "S2"):
        ps = short_pairs(s)
        assert any(len(p.cigar) > 16 for p in ps) or sum(len(p.cigar) for p in ps) > 16
        got = run(engine, ps)
        assert got > ladder_launches(max(p.band for p in ps)), "scheme %s: %d launches -- the pool was never regrown" % (s, got)
        n += len(ps)
    return n


def check_switches(make_engine):
    """the code paths that ordinary inputs do not reach, one context per variant (a context reads its switches when it is created, and says in
    tuning() what it read): DP rows of the wide kernel in global memory at every band up to 255 (gap, shift, edge and the random fillers), and a
    CIGAR pool of 16 words that is regrown, and the ladder restarted, several times per batch; returns the number of pairs checked"""
    variants = [("SMR_TRACE_GLOBAL_ROWS", "1", 1, lambda e: check(e, ("gap", "shift", "edge", "fill"), max_band=255)),
                ("SMR_CIGAR_POOL_WORDS", "16", 16, check_pool_of_16_words)]
    n = 0
    try:
        for name, value, read_as, body in variants:
            for k, _, _, _ in variants:
                os.environ.pop(k, None)
            os.environ[name] = value
            engine = make_engine()
            try:
                assert engine.tuning()[name] == read_as
                n += body(engine)
            finally:
                engine.close()
    finally:
        for k, _, _, _ in variants:
            os.environ.pop(k, None)
    return n
