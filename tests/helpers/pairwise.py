"""Batches with explicit CIGARs and the host writer's answer for the tests of smr_pairwise_part (test_gpu_pairwise.py / test_emu_pairwise.py).
TEST INFRASTRUCTURE ONLY.

The yardstick is always smr_report_add of a report opened with blast_pairwise: the same reads and records go through it into a temporary
directory, and the aligned.blast it wrote is compared with the device's streams for equality."""
import os
import re

import numpy as np

from sortmerna_amd import report

from . import fastx, rows

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
# (name, CIGAR as [(length, 0 M | 1 I | 2 D)], ref_begin1, letters clipped in front, strand, key, score or None, special letters)
M, I, D = 0, 1, 2
COLUMN_CASES = (
    [("m%d" % n, [(n, M)], 17 + n, 0, n & 1, (0, 0), None, "") for n in (1, 59, 60, 61, 119, 120, 121)] +
    [("i_straddle", [(57, M), (5, I), (30, M)], 30, 0, 1, (0, 0), None, ""), ("d_straddle", [(57, M), (5, D), (30, M)], 31, 0, 0, (0, 0), None, ""),
     ("i_ends60", [(55, M), (5, I), (20, M)], 32, 0, 0, (0, 0), None, ""), ("d_ends60", [(55, M), (5, D), (20, M)], 33, 0, 1, (0, 0), None, ""),
     ("i_begins60", [(60, M), (5, I), (20, M)], 34, 0, 1, (0, 0), None, ""), ("d_begins60", [(60, M), (5, D), (20, M)], 35, 0, 0, (0, 0), None, ""),
     ("i_begins60b", [(59, M), (5, I), (20, M)], 44, 0, 0, (0, 0), None, ""), ("d_begins60b", [(59, M), (5, D), (20, M)], 45, 0, 1, (0, 0), None, ""),
     ("i_chunk", [(60, M), (60, I), (10, M)], 36, 0, 1, (0, 0), None, ""), ("d_chunk", [(60, M), (60, D), (10, M)], 37, 0, 0, (0, 0), None, ""),
     ("i_first_chunk", [(60, I), (10, M)], 0, 0, 1, (0, 0), None, ""),
     ("i_ends", [(3, I), (40, M), (4, I)], 38, 0, 1, (0, 0), None, ""), ("d_ends", [(3, D), (40, M), (4, D)], 39, 0, 0, (0, 0), None, ""),
     ("i_ends_rev", [(3, I), (70, M), (4, I)], 40, 2, 0, (0, 0), None, "")] +
    [("digits%d" % rb, [(70, M)], rb, 0, rb & 1, (0, 0), None, "") for rb in (8, 9, 39, 40, 98, 99, 939, 940, 998, 999)] +
    [("clip", [(50, M), (2, D), (30, M)], 200, 7, 1, (0, 0), None, ""), ("clip_rev", [(50, M), (2, I), (30, M)], 201, 11, 0, (0, 0), None, ""),
     ("letters", [(80, M)], 300, 0, 1, (0, 0), None, "NnuUacgt"), ("letters_rev", [(80, M)], 301, 0, 0, (0, 0), None, "NnuUacgt"),
     ("other_part", [(65, M)], 50, 0, 1, (0, 1), None, ""), ("other_index", [(65, M)], 51, 0, 0, (1, 0), None, ""),
     ("high_score", [(65, M)], 52, 3, 1, (0, 0), 60000, ""),
     # operations without columns (imported state may hold them): a chunk whose columns lie more than 64 operations apart
     ("zero_ops", [(10, M)] + [(0, I), (0, D)] * 40 + [(70, M), (0, D)], 60, 0, 1, (0, 0), None, ""),
     ("zero_ops_rev", [(0, I)] * 70 + [(59, M)] + [(0, M)] * 65 + [(3, I), (0, D), (30, M)], 61, 1, 0, (0, 0), None, "")])


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def column_batch(ref_seqs, cases=COLUMN_CASES, fastq=False, slots=2, ref_of=None):
    """-> (FASTX text, records, slots): one read with one alignment per case.  The read's letters are the reference's along the CIGAR with every
    seventh column changed (a '*' mark), random at insertions; `special` letters replace the first ones (the printed letter: N, or the same)"""
    rng = np.random.Generator(np.random.PCG64(11))
    text, recs = [], []
    for j, (name, ops, rb, front, strand, key, score, special) in enumerate(cases):
        ref_num = ref_of(j) if ref_of else j % len(ref_seqs)
        ref = ref_seqs[ref_num].upper().replace("U", "T")
        shown, q, col = "", rb, 0                    # the letters of the Query lines, in their order
        for n, op in ops:
            for _ in range(n):
                if op == M:
                    c = ref[q]
                    c = c if c in "ACGT" else "A"
                    shown += "ACGT"[("ACGT".index(c) + 1) % 4] if col % 7 == 3 else c
                    q += 1
                elif op == I:
                    shown += "ACGT"[int(rng.integers(0, 4))]
                else:
                    q += 1
                col += 1
        assert q <= len(ref), name
        back = 2 if front else 0
        shown = "ACGT"[j % 4] * front + shown + "GT"[:back]
        seq = shown if strand else revcomp(shown)
        seq = special + seq[len(special):]
        used = len(shown) - front - back
        aln = dict(cigar=[(n << 4) | op for n, op in ops], ref_num=ref_num, ref_begin1=rb, ref_end1=q - 1, read_begin1=front, read_end1=front + used - 1,
                   readlen=len(seq), score1=(40 + j) if score is None else score, part=key[1], index_num=key[0], strand=strand)
        qual = "".join(chr(33 + (5 * k + j) % 41) for k in range(len(seq)))
        text.append(("@%s extra words\n%s\n+\n%s\n" % (name, seq, qual)) if fastq else (">%s extra words\n%s\n" % (name, seq)))
        recs.append(rows.record([aln], slots))
    return "".join(text).encode(), recs, slots


def open_report(tmpdir, fastq, reg, dbs=rows.DB, sam=False, tabular=False):
    os.makedirs(str(tmpdir), exist_ok=True)
    rep = report.Report(str(tmpdir), is_fastq=fastq, fastx=False, other=False, blast_pairwise=True, sam=sam, blast_cols=[] if tabular else None)
    for k, (lam, K, fr, fq) in dbs.items():
        rep.set_db(k, lam, K, fr, fq)
    for (k, part), ix in reg.items():
        rep.set_part(k, part, ix)
    return rep


def blast_file(tmpdir):
    return open(os.path.join(str(tmpdir), "aligned.blast"), "rb").read()


def host_file(tmpdir, reads, recs, fastq, reg, dbs=rows.DB):
    """the per-read host loop: smr_reads_record_text + smr_report_add -> aligned.blast as bytes"""
    rep = open_report(tmpdir, fastq, reg, dbs)
    for i, rec in enumerate(recs):
        hdr, seq, qual = reads.record_text(i)
        rep.add(hdr, seq, qual, rec)
    rep.close()
    return blast_file(tmpdir)


def device_file(tmpdir, e, fastq, reg, params_of, dbs=rows.DB, slot_of=None, streams=None, feed=None):
    """smr_pairwise_part per (index, part) + smr_report_add_pairwise, in a report that skips its own pairwise text -> aligned.blast; streams (a
    dict) gets the device's bytes per key; feed = (reads, recs): the reads go through smr_report_add as well, which must add nothing"""
    rep = open_report(tmpdir, fastq, reg, dbs)
    rep.skip_pairwise()
    for key, ix in reg.items():
        p = params_of(key)
        p.index_num, p.part = key
        lam, K, fr, fq = dbs[key[0]]
        data = e.pairwise_part(slot_of(key, ix) if slot_of else 0, p, ix, lam=lam, K=K, full_ref=fr, full_read=fq)
        if streams is not None:
            streams[key] = data
        rep.add_pairwise(key[0], key[1], data)
    if feed:
        for i, rec in enumerate(feed[1]):
            hdr, seq, qual = feed[0].record_text(i)
            rep.add(hdr, seq, qual, rec)
    rep.close()
    return blast_file(tmpdir)


_TARGET = re.compile(r"^Target: +(\d+)    ([ACGTN-]+)    (-?\d+)$")
_QUERY = re.compile(r"^Query: +(\d+)    ([ACGTN-]+)    (\d+)$")


def parse(text):
    """the blocks of a pairwise text -> [dict(ref, query, score, strand, start = byte offset, chunks = [(first, letters, last, marks, first,
    letters, last)])]; asserts the layout of every line on the way"""
    out, at = [], 0
    lines = text.decode().split("\n")
    k = 0
    while k < len(lines) - 1:
        assert lines[k].startswith("Sequence ID: ") and lines[k + 1].startswith("Query ID: ") and lines[k + 2].startswith("Score: ") and lines[k + 3] == "", (k, lines[k:k + 4])
        b = dict(ref=lines[k][13:], query=lines[k + 1][10:], score=int(lines[k + 2].split()[1]), strand=lines[k + 2][-1], start=at, chunks=[])
        at += sum(len(l) + 1 for l in lines[k:k + 4])
        k += 4
        while k < len(lines) - 1 and lines[k].startswith("Target: "):
            t, q = _TARGET.match(lines[k]), _QUERY.match(lines[k + 2])
            assert t and q and lines[k + 3] == "", lines[k:k + 4]
            n = len(t.group(2))
            assert len(lines[k]) - len(lines[k].rstrip("0123456789")) == len(t.group(3)) and len(q.group(2)) == n <= 60
            assert lines[k + 1][:20] == " " * 20 and len(lines[k + 1]) == 20 + n and set(lines[k + 1][20:]) <= set("|* ")
            assert len(lines[k]) == 8 + max(8, len(t.group(1))) + 4 + n + 4 + len(t.group(3)) and len(lines[k + 2]) == 7 + max(9, len(q.group(1))) + 4 + n + 4 + len(q.group(3))
            b["chunks"].append((int(t.group(1)), t.group(2), int(t.group(3)), lines[k + 1][20:], int(q.group(1)), q.group(2), int(q.group(3))))
            at += sum(len(l) + 1 for l in lines[k:k + 4])
            k += 4
        assert b["chunks"], b
        out.append(b)
    assert at == len(text) and lines[-1] == ""
    return out
