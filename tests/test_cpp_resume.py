"""The C++ streaming host (examples/smr_align_mgpu.cpp) with --state-out / --state-in: a run over the first database writes the stored state
of every read, a second process continues it on the second database, chunk by chunk (every chunk imports its slice of the records before its
first part).  The final records must be those of two contexts of the library driven the same way (test_gpu_state_import.py, which checks
them against the oracle); a state file written for other reads is refused before anything is aligned."""
import os
import struct
import subprocess

import pytest

from helpers import golden, refrun
from test_cpp_driver import build_mgpu
from test_gpu_state_import import resume_finished

pytestmark = pytest.mark.gpu
CASE = "two_db_default"


def _cmd(exe, out, k, extra):
    g = golden.load()[CASE]
    dbs, rd, _ = golden.inputs(CASE)
    return [exe, "--reads", rd, "--out", str(out), "--ref", dbs[k], "--gumbel", repr(g["log"]["lambda"][k]), repr(g["log"]["K"][k]), "--chunk-reads", "150"] + extra


def test_a_run_written_out_after_db1_is_continued_on_db2(tmp_path):
    exe = build_mgpu()
    g = golden.load()[CASE]
    _, _, seqs = golden.inputs(CASE)
    assert len(seqs) > 4 * 150                            # several chunks, the last one short
    d1, d2, state = tmp_path / "db1", tmp_path / "db2", str(tmp_path / "run.state")
    d1.mkdir(), d2.mkdir()
    subprocess.check_call(_cmd(exe, d1, 0, ["--state-out", state]))
    recs_a, recs_b, _, _, _, _ = resume_finished(0, CASE)
    # the state file: header, counters of DB 1, offsets, the records of the first half
    blob = open(state, "rb").read()
    assert blob[:9] == b"SMRSTATE1"
    n, _, n_db = struct.unpack_from("<3Q", blob, 9)
    assert (n, n_db) == (len(seqs), 1)
    ctr = struct.unpack_from("<3Q", blob, 33)
    off = struct.unpack_from("<%dQ" % (n + 1), blob, 57)
    body = blob[57 + 8 * (n + 1):]
    assert len(body) == off[n] and [body[off[i]:off[i + 1]] for i in range(n)] == recs_a
    assert ctr[0] == ctr[2] == g["readstats"]["reads_matched_per_db"][0]
    # a file for other reads: refused, nothing aligned, nothing written
    wrong = str(tmp_path / "wrong.state")
    open(wrong, "wb").write(blob[:17] + bytes([blob[17] ^ 1]) + blob[18:])
    p = subprocess.run(_cmd(exe, d2, 1, ["--state-in", wrong]), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"ERROR" in p.stderr and b"other reads" in p.stderr, p.stderr
    assert b"[timing]" not in p.stdout and not os.listdir(d2)
    fewer = str(tmp_path / "fewer.state")
    open(fewer, "wb").write(blob[:9] + struct.pack("<Q", n - 1) + blob[17:])
    p = subprocess.run(_cmd(exe, d2, 1, ["--state-in", fewer]), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"ERROR" in p.stderr and not os.listdir(d2), p.stderr
    # the second process
    out = subprocess.check_output(_cmd(exe, d2, 1, ["--state-in", state, "--state-out", str(tmp_path / "run2.state")])).decode()
    assert "[timing]" in out
    kv = refrun.parse_kvdb_dump(str(d2 / "records.bin"))
    assert len(kv) == sum(1 for r in recs_b if r)
    bad = [i for i in range(n) if kv.get(b"0_%d" % i, b"") != recs_b[i]]
    assert not bad, "%d records differ, first %d" % (len(bad), bad[0])
    summary = open(d2 / "summary.txt").read()
    assert "Total reads passing E-value threshold = %d\n" % g["readstats"]["num_aligned"] in summary
    assert "%s\t%d\n" % (golden.inputs(CASE)[0][1], g["readstats"]["reads_matched_per_db"][1]) in summary
    n2, _, n_db2 = struct.unpack_from("<3Q", open(tmp_path / "run2.state", "rb").read(), 9)
    assert (n2, n_db2) == (n, 2)
