"""Fixtures of the %id / %coverage pass: what the UNMODIFIED reference writes under -otu_map / -de_novo_otu / -id / -coverage on
inputs already committed under tests/golden/ (written by make_golden.py).

    python tests/golden/make_golden_otu.py      # rewrites tests/golden/otu/*

Per case: <case>.records.bin = the per-read KVDB values AFTER denovo_stats (Read::toBinString bytes with c_yid_ycov, n_yid_ncov,
n_nid_ycov, n_denovo filled in; same container as ../*.records.bin), <case>.otu_map.txt (absent when the reference wrote none),
<case>.denovo.fa = aligned_denovo.fa, <case>.log.txt = aligned.log (paths rewritten relative to tests/golden/ as make_golden_reports2.py
does), and in otu.json the options, thresholds, hot-path parameters and the four totals of the reference's `num_yid_ycov: ...` log line.
The script refuses to write a case in which fewer than two of the four classes occur (except the thresholds-0 case, where everything
passes by construction): a regenerated fixture cannot silently become trivial.
The paired cases (the two mate files of make_golden_paired.py under -paired_in / -out2 / -sout): the records after denovo_stats, mate 1 and
mate 2 alternating, and the read ids of every aligned_denovo* file the reference wrote."""
import json
import os
import re
import shutil
import struct
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, REPO)

from helpers import golden, paths, refrun  # noqa: E402

OTU = ["-otu_map", "-de_novo_otu"]
# name -> (golden case whose inputs are used, extra options, hot-path parameters for smr.default_params, (min_id, min_cov), trivial allowed)
CASES = {
    "syn": ("syn_default", OTU + ["-id", "0.97", "-coverage", "0.97"], {}, (0.97, 0.97), False),
    "syn_all": ("syn_all", OTU + ["-id", "0.97", "-coverage", "0.97", "-num_alignments", "0"], {"num_alignments": 0}, (0.97, 0.97), False),
    "real": ("real_default", OTU + ["-id", "0.97", "-coverage", "0.97"], {}, (0.97, 0.97), False),
    "two_db": ("two_db_default", OTU + ["-id", "0.9", "-coverage", "0.5"], {}, (0.9, 0.5), False),
    "syn_denovo_only": ("syn_default", ["-de_novo_otu"], {}, (0.0, 0.0), True),
    "syn_multipart": ("syn_multipart", OTU + ["-m", "0.15"], {"max_mb": 0.15}, (0.97, 0.97), False),
}


PAIRED = {"paired_in": ["-paired_in"], "paired_out2": ["-out2"], "paired_sout": ["-sout"], "paired_out2_sout": ["-out2", "-sout"], "paired_plain": [],
          # looser thresholds, so that mates reach the map: the order of the two mates of a pair within a group
          "paired_loose": ["-id", "0.9", "-coverage", "0.5"], "paired_loose_in": ["-id", "0.9", "-coverage", "0.5", "-paired_in"]}


def write_records(path, recs):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)))
        for r in recs:
            f.write(struct.pack("<I", len(r)))
            f.write(r)


def main():
    assert paths.have_reference() and paths.have_ref_bin(), "needs the reference sources and oracle/_ref/sortmerna_ref (make -C oracle ref)"
    out = os.path.join(HERE, "otu")
    os.makedirs(out, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix="golden_otu_")
    G = {}
    for name, (src, extra, params, thr, trivial_ok) in CASES.items():
        dbs, rd, seqs = golden.inputs(src)
        if not isinstance(dbs, list):
            dbs = [dbs]
        wd = os.path.join(tmp, name)
        res = refrun.run_reference(dbs, [rd], wd, extra=list(extra) + ["-fastx", "-v"], threads=1)
        assert res.rc == 0, res.stdout[-3000:]
        m = re.search(r"num_yid_ycov: (\d+)\s+num_yid_ncov: (\d+)\s+num_nid_ycov: (\d+)\s+num_denovo: (\d+)", res.stdout)
        assert m, "no denovo_stats line in the reference's output"
        totals = [int(x) for x in m.groups()]
        assert trivial_ok or sum(1 for t in totals if t) >= 2, (name, totals)
        recs = [res.kvdb.get(b"0_%d" % i, b"") for i in range(len(seqs))]
        per_read = [0, 0, 0, 0]
        for r in recs:
            if r:
                for k, v in enumerate(struct.unpack_from("<4I", r, 8)):
                    per_read[k] += v
        assert per_read == totals, (name, per_read, totals)          # the dump was taken after denovo_stats
        write_records(os.path.join(out, name + ".records.bin"), recs)
        o = os.path.join(wd, "out")
        fix = lambda t: t.replace(HERE + "/", "").replace(wd, "WORKDIR").replace(paths.REF_BIN, "sortmerna")
        g = dict(inputs=src, options=extra, params=params, min_id=thr[0], min_cov=thr[1], totals=totals, records=name + ".records.bin", otu_map=None, n_groups=0)
        mp = os.path.join(o, "otu_map.txt")
        if os.path.isfile(mp):
            shutil.copyfile(mp, os.path.join(out, name + ".otu_map.txt"))
            g["otu_map"] = name + ".otu_map.txt"
            g["n_groups"] = sum(1 for _ in open(mp))
        elif os.path.isfile(os.path.join(out, name + ".otu_map.txt")):
            os.remove(os.path.join(out, name + ".otu_map.txt"))
        shutil.copyfile(os.path.join(o, "aligned_denovo.fa"), os.path.join(out, name + ".denovo.fa"))
        open(os.path.join(out, name + ".log.txt"), "w").write(fix(open(os.path.join(o, "aligned.log")).read()))
        G[name] = g
        print(name, "totals", totals, "groups", g["n_groups"], "denovo reads", sum(1 for l in open(os.path.join(out, name + ".denovo.fa")) if l.startswith(">")))
    # ---- paired reads (the mate files of make_golden_paired.py against real_db.fasta): which read goes to which aligned_denovo file ----
    rd = [os.path.join(HERE, "paired", "paired_%d.fastq" % k) for k in (1, 2)]
    n_pairs = sum(1 for _ in open(rd[0])) // 4
    for name, extra in PAIRED.items():
        wd = os.path.join(tmp, name)
        res = refrun.run_reference([os.path.join(HERE, "real_db.fasta")], rd, wd, extra=OTU + ["-fastx", "-v"] + extra, threads=1)
        assert res.rc == 0, res.stdout[-3000:]
        m = re.search(r"num_yid_ycov: (\d+)\s+num_yid_ncov: (\d+)\s+num_nid_ycov: (\d+)\s+num_denovo: (\d+)", res.stdout)
        totals = [int(x) for x in m.groups()]
        assert sum(1 for t in totals if t) >= 2, (name, totals)
        recs = []
        for i in range(n_pairs):
            recs.append(res.kvdb.get(b"0_%d" % i, b""))
            recs.append(res.kvdb.get(b"1_%d" % i, b""))
        write_records(os.path.join(out, name + ".records.bin"), recs)
        o = os.path.join(wd, "out")
        files = {fn: [l.split()[0][1:] for l in open(os.path.join(o, fn)).readlines()[0::4]] for fn in sorted(os.listdir(o)) if fn.startswith("aligned_denovo")}
        assert any(files.values()), name
        loose = "-id" in extra
        if loose:
            assert totals[0] > 0 and os.path.isfile(os.path.join(o, "otu_map.txt")), (name, totals)
            shutil.copyfile(os.path.join(o, "otu_map.txt"), os.path.join(out, name + ".otu_map.txt"))
        G[name] = dict(paired=True, options=OTU + extra, min_id=0.9 if loose else 0.97, min_cov=0.5 if loose else 0.97, totals=totals, records=name + ".records.bin", denovo_files=files,
                       otu_map_exists=os.path.isfile(os.path.join(o, "otu_map.txt")))
        print(name, "totals", totals, {k: len(v) for k, v in files.items()})
    json.dump(G, open(os.path.join(out, "otu.json"), "w"), indent=1, sort_keys=True)
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
