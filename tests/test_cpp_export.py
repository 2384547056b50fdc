"""The C++ streaming host (examples/smr_align_mgpu.cpp) with --records bulk: every chunk's records come from one smr_state_export into a host
buffer of its batch slot, and the writer thread slices that buffer for the report rows, the key-value dump and --state-out instead of
serialising read after read.  Every file the run writes must be byte-identical to the default (--records per-read) run's."""
import filecmp
import os
import subprocess

import pytest

from helpers import golden
from test_cpp_driver import build_mgpu

pytestmark = pytest.mark.gpu
CASE = "two_db_default"


def _run(exe, out, state, extra):
    g = golden.load()[CASE]
    dbs, rd, _ = golden.inputs(CASE)
    cmd = [exe, "--reads", rd, "--out", str(out), "--chunk-reads", "150", "--fastx", "--other", "--blast", "1 cigar qcov qstrand", "--sam", "--state-out", state]
    for k, db in enumerate(dbs):
        cmd += ["--ref", db, "--gumbel", repr(g["log"]["lambda"][k]), repr(g["log"]["K"][k])]
    return subprocess.check_output(cmd + extra).decode()


def _files(root):
    return sorted(os.path.relpath(os.path.join(d, f), root) for d, _, fs in os.walk(root) for f in fs)


def test_bulk_records_give_the_files_of_the_per_read_path(tmp_path):
    exe = build_mgpu()
    _, _, seqs = golden.inputs(CASE)
    assert len(seqs) > 4 * 150                            # several chunks, the last one short
    a, b = tmp_path / "per_read", tmp_path / "bulk"
    a.mkdir(), b.mkdir()
    sa, sb = str(tmp_path / "a.state"), str(tmp_path / "b.state")
    assert "[timing]" in _run(exe, a, sa, [])
    assert "[timing]" in _run(exe, b, sb, ["--records", "bulk"])
    fa = _files(a)
    assert fa == _files(b)
    for want in ("aligned.blast", "aligned.sam", "records.bin"):
        assert any(f.endswith(want) for f in fa), (want, fa)
    assert any("aligned.f" in f for f in fa) and any("other.f" in f for f in fa), fa
    differ = [f for f in fa if not filecmp.cmp(a / f, b / f, shallow=False)]
    assert not differ, differ
    assert os.path.getsize(sa) > 1000 and filecmp.cmp(sa, sb, shallow=False)
    # an unknown setting is refused before anything runs
    p = subprocess.run([exe, "--records", "sometimes"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0 and b"--records" in p.stderr
