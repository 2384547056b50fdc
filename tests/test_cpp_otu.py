"""The C++ streaming host (examples/smr_align_mgpu.cpp) under -otu_map / -de_novo_otu / -id / -coverage: the %id / %coverage pass per chunk
after the traceback, its four sums in the counter reduction, the OTU map merged over chunks and ranks before it is written.  otu_map.txt,
aligned_denovo.fa and aligned.log must be the files the unmodified reference wrote (tests/golden/otu/), with a chunk size that splits the
input into several chunks and with several ranks; the reference's two option refusals exit non-zero with a message."""
import os
import subprocess

import pytest

from helpers import golden, otu, paths, refrun
from test_cpp_driver import build_mgpu


def _run(case, tmp_path, extra):
    g = otu.load()[case]
    gg = golden.load()[g["inputs"]]
    dbs, rd, seqs = golden.inputs(g["inputs"])
    if not isinstance(dbs, list):
        dbs = [dbs]
    # (paths relative to tests/golden, as the fixtures' aligned.log prints them)
    cmd = [build_mgpu(), "--reads", os.path.basename(rd), "--out", str(tmp_path), "-fastx"] + list(g["options"]) + extra
    for k, db in enumerate(dbs):
        cmd += ["--ref", os.path.basename(db), "--gumbel", repr(gg["log"]["lambda"][k]), repr(gg["log"]["K"][k])]
    out = subprocess.check_output(cmd, cwd=paths.GOLDEN).decode()
    assert "[timing]" in out
    # the per-read records after the pass are the reference's after denovo_stats
    kv = refrun.parse_kvdb_dump(str(tmp_path / "records.bin"))
    want = otu.records(case)
    bad = [i for i in range(len(seqs)) if kv.get(b"0_%d" % i, b"") != want[i]]
    assert not bad, "%d records differ, first %d" % (len(bad), bad[0])
    # the three files
    assert os.path.isfile(tmp_path / "otu_map.txt") == (g["otu_map"] is not None)
    if g["otu_map"]:
        assert open(tmp_path / "otu_map.txt", "rb").read() == open(os.path.join(otu.OTU_DIR, g["otu_map"]), "rb").read()
    assert open(tmp_path / "aligned_denovo.fa", "rb").read() == open(os.path.join(otu.OTU_DIR, case + ".denovo.fa"), "rb").read()
    got = open(tmp_path / "aligned.log").read().split("\n")
    exp = open(os.path.join(otu.OTU_DIR, case + ".log.txt")).read().split("\n")
    assert len(got) == len(exp)
    own = {1, len(exp) - 3}                 # the command line and the ctime() line are each program's own
    if "--gpus" in extra:
        own.add([i for i, l in enumerate(exp) if l.startswith("    Number of alignment processing threads")][0])      # = ranks here
    assert [l for i, l in enumerate(got) if i not in own] == [l for i, l in enumerate(exp) if i not in own]
    summary = open(tmp_path / "summary.txt").read()
    t = g["totals"]
    assert "num_yid_ycov = %d\nnum_yid_ncov = %d\nnum_nid_ycov = %d\nnum_denovo = %d\nTotal OTUs = %d\n" % (t[0], t[1], t[2], t[3], g["n_groups"]) in summary
    assert not [d for d in os.listdir(tmp_path) if d.startswith("rank")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["syn", "two_db", "real"])
def test_one_rank_several_chunks(case, tmp_path):
    _run(case, tmp_path, ["--chunk-reads", "100"])          # 360 .. 510 reads: four to six chunks through three recycled batch slots


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["syn", "two_db"])
def test_three_ranks_on_one_device_merge_their_maps(case, tmp_path):
    _run(case, tmp_path, ["--gpus", "3", "--devices", "0,0,0", "--reduce", "host", "--chunk-reads", "70"])


def test_the_reference_s_option_refusals(tmp_path):
    """options.cpp:1623-1628, 1667-1674, 1744-1757: -id / -coverage only with -otu_map; -otu_map not with -no-best (said before any device is touched)"""
    exe = build_mgpu()
    base = [exe, "--ref", "syn_db.fasta", "--gumbel", "0.6", "0.33", "--reads", "syn_reads.fasta", "--out", str(tmp_path)]
    for extra, word in ((["-id", "0.9"], "-otu_map"), (["-coverage", "0.9"], "-otu_map"), (["-de_novo_otu", "-id", "0.9"], "-otu_map"), (["-otu_map", "-no-best"], "-no-best"),
                        (["-otu_map", "-id", "1.5"], "[0, 1]")):
        p = subprocess.run(base + extra, cwd=paths.GOLDEN, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert p.returncode != 0 and b"ERROR" in p.stderr and word.encode() in p.stderr, (extra, p.stderr)
