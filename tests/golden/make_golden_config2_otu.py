"""BASELINE config 2 at full size under -otu_map -de_novo_otu (the reference's defaults 0.97 / 0.97, and once more with -id 0.9 -coverage 0.5): the 100 000 bundled amplicon reads
against silva-arc-16s-id95 through the UNMODIFIED reference binary, one thread.  Written into tests/golden/config2/config2_otu.json: MD5
digests of the per-read records AFTER denovo_stats (per 1000 reads + total, as make_golden_config2.py does), the four totals of the
reference's denovo_stats log line, the number of OTU groups, and the MD5 of otu_map.txt (null when the reference wrote none) and of aligned_denovo.fa.

    python tests/golden/make_golden_config2_otu.py      # needs the reference sources and `make -C oracle ref`; a few minutes
"""
import gzip
import hashlib
import json
import os
import re
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from helpers import fastx, paths, refrun  # noqa: E402
from make_golden_config2 import CHUNK, OUT, digests  # noqa: E402


def main():
    base = json.load(open(os.path.join(OUT, "config2.json")))
    tmp = tempfile.mkdtemp(prefix="smr_c2otu_")
    flat, db = os.path.join(tmp, "reads.fasta"), os.path.join(tmp, base["db"][:-3])
    for src, dst in ((base["reads"], flat), (base["db"], db)):
        with gzip.open(os.path.join(OUT, src), "rb") as f, open(dst, "wb") as g:
            g.write(f.read())
    n = len(fastx.read_fastx(flat))
    assert n == base["n_reads"]
    md5 = lambda p: hashlib.md5(open(p, "rb").read()).hexdigest()
    out = {"n_reads": n, "chunk": CHUNK, "runs": {}}
    # the issue's run (the reference's defaults 0.97 / 0.97 under -otu_map) and a looser pair of thresholds, so that a map is written at this size
    for name, extra, thr in (("default", [], (0.97, 0.97)), ("id90_cov50", ["-id", "0.9", "-coverage", "0.5"], (0.9, 0.5))):
        res = refrun.run_reference([db], [flat], os.path.join(tmp, "wd_" + name), extra=["-otu_map", "-de_novo_otu", "-fastx", "-v"] + extra, threads=1, timeout=7200)
        assert res.rc == 0, res.stdout[-2000:]
        m = re.search(r"num_yid_ycov: (\d+)\s+num_yid_ncov: (\d+)\s+num_nid_ycov: (\d+)\s+num_denovo: (\d+)", res.stdout)
        totals = [int(x) for x in m.groups()]
        assert sum(1 for t in totals if t) >= 2, totals
        recs = [res.kvdb.get(b"0_%d" % i, b"") for i in range(n)]
        tot, chunks = digests(recs)
        o = os.path.join(tmp, "wd_" + name, "out")
        mp = os.path.join(o, "otu_map.txt")
        have = os.path.isfile(mp)
        assert have == (totals[0] > 0)                      # otumap.cpp:200,276
        out["runs"][name] = {"options": ["-otu_map", "-de_novo_otu"] + extra, "min_id": thr[0], "min_cov": thr[1], "totals": totals,
                             "lambda": res.log["lambda"][0], "K": res.log["K"][0], "minimal_score": res.log["minimal_score"][0], "num_aligned": res.log["num_aligned"],
                             "n_records": sum(1 for r in recs if r), "md5_total": tot, "md5_chunks": chunks,
                             "n_groups": sum(1 for _ in open(mp)) if have else 0, "md5_otu_map": md5(mp) if have else None,
                             "n_denovo_reads": sum(1 for l in open(os.path.join(o, "aligned_denovo.fa")) if l.startswith(">")), "md5_denovo": md5(os.path.join(o, "aligned_denovo.fa"))}
        print(name, {k: v for k, v in out["runs"][name].items() if k != "md5_chunks"})
    json.dump(out, open(os.path.join(OUT, "config2_otu.json"), "w"), indent=0)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
