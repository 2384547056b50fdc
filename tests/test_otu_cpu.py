"""CPU: the writers behind -otu_map / -de_novo_otu (smr_report: otu_map.txt, aligned_denovo.fa|fq; smr_summary_write: the two optional
Results lines) fed with the reference's own per-read records AFTER its denovo_stats must reproduce, byte for byte, what the unmodified
reference wrote (tests/golden/otu/, tests/golden/make_golden_otu.py): fill_otu_map2 / OtuMap::write otumap.cpp:72-281,
ReportDenovo::append report_denovo.cpp:57-134, Summary::to_string summary.cpp:102-175."""
import gzip
import os
import struct

import pytest

import sortmerna_amd as smr
from sortmerna_amd import report
from helpers import fastx, golden, otu, paths

SINGLE = ["syn", "syn_all", "real", "two_db", "syn_denovo_only", "syn_multipart"]
PAIRED = ["paired_plain", "paired_in", "paired_out2", "paired_sout", "paired_out2_sout", "paired_loose", "paired_loose_in"]


def _write(case, out_dir, zip_out=False):
    g = otu.load()[case]
    src = g["inputs"]
    gg = golden.load()[src]
    dbs, rd, _ = golden.inputs(src)
    if not isinstance(dbs, list):
        dbs = [dbs]
    recs = otu.records(case)
    reads = fastx.read_fastx(rd)
    assert len(reads) == len(recs)
    is_otu, is_dn = "-otu_map" in g["options"], "-de_novo_otu" in g["options"]
    rep = report.Report(str(out_dir), is_fastq=False, fastx=False, other=False, otu_map=is_otu, denovo=is_dn, min_id=g["min_id"], min_cov=g["min_cov"], zip_out=zip_out)
    keep = []
    for k, db in enumerate(dbs):
        parts = smr.Index.build(db, 18, gg["params"].get("max_mb", 3072.0), 10000, 0)
        keep += parts
        for j, ix in enumerate(parts):
            rep.set_part(k, j, ix)
    for (hdr, seq, qual), rec in zip(reads, recs):
        rep.add(hdr, seq, qual, rec)
    rep.close()
    for ix in keep:
        ix.free()
    return g, gg, dbs, rd, rep.total_otu


@pytest.mark.parametrize("case", SINGLE)
def test_otu_map_denovo_file_and_summary_equal_the_reference(case, tmp_path):
    g, gg, dbs, rd, total_otu = _write(case, tmp_path)
    have = os.path.isfile(tmp_path / "otu_map.txt")
    assert have == (g["otu_map"] is not None)               # no file at all when no read passed both thresholds (otumap.cpp:200,276)
    if have:
        assert open(tmp_path / "otu_map.txt", "rb").read() == open(os.path.join(otu.OTU_DIR, g["otu_map"]), "rb").read()
    assert total_otu == g["n_groups"]
    assert open(tmp_path / "aligned_denovo.fa", "rb").read() == open(os.path.join(otu.OTU_DIR, case + ".denovo.fa"), "rb").read()
    # aligned.log: the command line and the ctime() line are the reference's own text, handed through; the pid line of the fixture is empty
    log_exp = open(os.path.join(otu.OTU_DIR, case + ".log.txt")).read()
    lines = log_exp.split("\n")
    assert lines[3] == " Process pid = "
    rs, lg = gg["readstats"], gg["log"]
    is_otu, is_dn = "-otu_map" in g["options"], "-de_novo_otu" in g["options"]
    report.write_summary(str(tmp_path / "aligned.log"),
                         [dict(ref_file=os.path.basename(db), skiplengths=[18, 9, 3], lam=lg["lambda"][k], K=lg["K"][k], minimal_score=lg["minimal_score"][k],
                               reads_matched=rs["reads_matched_per_db"][k]) for k, db in enumerate(dbs)],
                         [os.path.basename(rd)], rs["all_reads_count"], rs["num_aligned"], rs["all_reads_len"], rs["min_read_len"], rs["max_read_len"],
                         threads=1, cmdline=lines[1][4:], pid="", timestamp=lines[-3].strip() + "\n",
                         total_denovo=g["totals"][3] if is_dn else None, total_id_cov=g["totals"][0] if is_otu else None, total_otu=total_otu)
    assert open(tmp_path / "aligned.log").read() == log_exp
    assert ("%%id and %%coverage" in log_exp) == is_otu and ("de novo clustering" in log_exp) == is_dn


def test_cases_cover_a_map_no_map_and_an_empty_denovo_file():
    G = otu.load()
    assert G["real"]["otu_map"] is None and G["real"]["totals"][0] == 0 and G["syn"]["n_groups"] == 35 and G["two_db"]["n_groups"] == 44
    assert os.path.getsize(os.path.join(otu.OTU_DIR, "syn_denovo_only.denovo.fa")) == 0


def test_without_the_options_nothing_new_is_written_and_the_summary_is_unchanged(tmp_path):
    recs, reads = otu.records("syn"), fastx.read_fastx(golden.inputs("syn_default")[1])
    rep = report.Report(str(tmp_path), is_fastq=False, fastx=True, other=False)
    for (hdr, seq, qual), rec in zip(reads, recs):
        rep.add(hdr, seq, qual, rec)
    rep.close()
    assert sorted(os.listdir(tmp_path)) == ["aligned.fa"] and rep.total_otu == 0


def test_gzip_denovo_file_holds_the_same_text_and_the_map_stays_plain(tmp_path):
    _write("two_db", tmp_path, zip_out=True)
    assert gzip.open(tmp_path / "aligned_denovo.fa.gz", "rb").read() == open(os.path.join(otu.OTU_DIR, "two_db.denovo.fa"), "rb").read()
    assert open(tmp_path / "otu_map.txt", "rb").read() == open(os.path.join(otu.OTU_DIR, "two_db.otu_map.txt"), "rb").read()


@pytest.mark.parametrize("case", PAIRED)
def test_paired_denovo_routing_equals_the_reference(case, tmp_path):
    g = otu.load()[case]
    m1 = fastx.read_fastx(os.path.join(paths.GOLDEN, "paired", "paired_1.fastq"))
    m2 = fastx.read_fastx(os.path.join(paths.GOLDEN, "paired", "paired_2.fastq"))
    recs = otu.records(case)
    assert len(recs) == 2 * len(m1) == 2 * len(m2)
    opt = g["options"]
    parts = smr.Index.build(os.path.join(paths.GOLDEN, "real_db.fasta"), 18, 3072.0, 10000, 0)
    rep = report.Report(str(tmp_path), is_fastq=True, fastx=False, other=False, otu_map=True, denovo=True, min_id=g["min_id"], min_cov=g["min_cov"],
                        paired_in="-paired_in" in opt, out2="-out2" in opt, sout="-sout" in opt)
    for j, ix in enumerate(parts):
        rep.set_part(0, j, ix)
    for i in range(len(m1)):
        rep.add_pair(m1[i] + (recs[2 * i],), m2[i] + (recs[2 * i + 1],))
    rep.close()
    for ix in parts:
        ix.free()
    got = {fn: [l.split()[0][1:] for l in open(tmp_path / fn).readlines()[0::4]] for fn in sorted(os.listdir(tmp_path)) if fn.startswith("aligned_denovo")}
    assert got == g["denovo_files"]
    assert os.path.isfile(tmp_path / "otu_map.txt") == g["otu_map_exists"]
    if g["otu_map_exists"]:
        # The looser thresholds.  With two mate files the reference's fill_otu_map2 reads `readfeed.next(id)` for id < threads only
        # (otumap.cpp:144), i.e. at -threads 1 the first mate file alone: mates of the second file never reach its map, whatever their
        # counters say (here its map file is empty: the one read that passed is a second mate).  That depends on the thread count and is
        # not reproduced: the map here holds every read with c_yid_ycov > 0, the reference's lines being those of the first mates.
        ours = [l.rstrip("\n").split("\t") for l in open(tmp_path / "otu_map.txt")]
        first_ids = {m[0].split()[0][1:] for m in m1}
        second_only = {m[0].split()[0][1:] for m in m2} - first_ids
        ref_lines = [l.rstrip("\n").split("\t") for l in open(os.path.join(otu.OTU_DIR, case + ".otu_map.txt"))]
        passed = [(i, struct.unpack_from("<4I", r, 8)[0]) for i, r in enumerate(recs) if r and struct.unpack_from("<4I", r, 8)[0] > 0]
        assert passed and sum(len(l) - 1 for l in ours) == sum(n for _, n in passed) and rep.total_otu == len(ours) > 0
        if not second_only:                 # (mates share their id in these files: the first-mate lines cannot be told apart by id)
            assert all(i % 2 == 1 for i, _ in passed) and ref_lines == []
        else:
            assert [[l[0]] + [x for x in l[1:] if x not in second_only] for l in ours if any(x not in second_only for x in l[1:])] == ref_lines
    # the records are copied verbatim
    by_id = {r[0].split()[0][1:]: r for r in m1 + m2}
    for fn, ids in got.items():
        lines = open(tmp_path / fn).read().split("\n")
        for k, rid in enumerate(ids[:10]):
            h, s, q = by_id[rid]
            assert lines[4 * k:4 * k + 4] == [h, s, "+", q]
