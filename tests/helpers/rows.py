"""Crafted batches and the host writer's answer for the tests of smr_rows_part (test_gpu_rows.py / test_emu_rows.py).  TEST INFRASTRUCTURE ONLY.

The yardstick is always smr_report_add: the same reads and records go through it into a temporary directory, and what it wrote is compared
with the device's streams for equality."""
import os
import struct

import numpy as np

from sortmerna_amd import report

from . import fastx

SYN_DB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "golden", "syn_db.fasta")
KEYS = [(0, 0), (0, 1), (1, 0)]                  # (index_num, part): the crafted records spread their alignments over these
DB = {0: (0.602, 0.33, 123456, 7890123), 1: (0.59, 0.41, 222222, 3333333)}       # lambda, K, full_ref_corr, full_read_corr per index
ALL_COLS = ["cigar", "qcov", "qstrand"]
# strands of the alignments of key (0, 0) within one read: the quality line is reversed in place at every 0
STRAND_SETS = [(0, 1), (0, 0), (1, 0, 0), (0, 1, 0), (1,), (0,), (1, 1), (1, 0)]
HEADERS = ["r%d", "r%d some words", "r%d\tTAB before a space", ">r%d", "@r%d x", "r%d ", "r%d  two"]


def ref_lengths(db=SYN_DB):
    return [len(s) for _, s, _ in fastx.read_fastx(db)]


def record(alns, num_alignments):
    """Read::toBinString bytes: alns = dicts(cigar, ref_num, ref_begin1, ref_end1, read_begin1, read_end1, readlen, score1, part, index_num, strand)"""
    if not alns:
        return b""
    body = b""
    for a in alns:
        cg = a["cigar"]
        body += struct.pack("<QQ", 39 + 4 * len(cg), len(cg)) + struct.pack("<%dI" % len(cg), *cg)
        body += struct.pack("<IiiiiI", a["ref_num"], a["ref_begin1"], a["ref_end1"], a["read_begin1"], a["read_end1"], a["readlen"])
        body += struct.pack("<HHHB", a["score1"], a["part"], a["index_num"], a["strand"])
    tail = struct.pack("<II", 0, 3) + struct.pack("<Q", len(alns)) + body
    head = struct.pack("<II4I", 0, 0, 0, 0, 0, 0) + struct.pack("<BBB", 1, 1, 0) + struct.pack("<H", 1) + struct.pack("<iI", num_alignments, 5)
    return head + struct.pack("<Q", len(tail)) + tail


def craft_alignment(rng, readlen, ref_lens, key, strand, clip, many_ops=False, score=None):
    """one alignment whose CIGAR stays inside the read and a reference; clip: 0 none, 1 front, 2 behind, 3 both"""
    front = int(rng.integers(1, 12)) if clip & 1 else 0
    back = int(rng.integers(1, 12)) if clip & 2 else 0
    front, back = min(front, readlen // 4), min(back, readlen // 4)
    room = max(ref_lens) - 64                       # a read longer than every reference: a longer clip in front
    if readlen - front - back > room:
        front = readlen - back - room
    left = readlen - front - back                   # read letters the CIGAR consumes
    ops, ref_used = [], 0
    if many_ops:
        while left > 0:
            m = min(left, int(rng.integers(1, 40)))
            ops.append((m, 0)); left -= m; ref_used += m
            if left > 2:
                if rng.integers(0, 2):
                    k = int(rng.integers(1, 3)); ops.append((k, 1)); left -= k
                else:
                    k = int(rng.integers(1, 3)); ops.append((k, 2)); ref_used += k
    else:
        kind = int(rng.integers(0, 4))
        if kind == 0 or left < 30:
            ops = [(left, 0)]; ref_used = left
        else:
            a = int(rng.integers(1, left - 20)); ins = int(rng.integers(1, 13)) if kind & 1 else 0; dele = int(rng.integers(1, 13)) if kind & 2 else 0
            b = left - a - ins
            ops = [(a, 0)] + ([(ins, 1)] if ins else []) + ([(dele, 2)] if dele else []) + [(b, 0)]
            ref_used = a + dele + b
    fits = [r for r, l in enumerate(ref_lens) if l >= ref_used + 1]
    ref_num = int(fits[int(rng.integers(0, len(fits)))])
    rb = int(rng.integers(0, ref_lens[ref_num] - ref_used + 1))
    return dict(cigar=[(n << 4) | op for n, op in ops], ref_num=ref_num, ref_begin1=rb, ref_end1=rb + ref_used - 1, read_begin1=front,
                read_end1=readlen - back - 1, readlen=readlen, score1=int(rng.integers(1, 2 * readlen)) if score is None else score,
                part=key[1], index_num=key[0], strand=strand)


def craft(n, fastq, ref_lens, seed=1, slots=6, long_read=False):
    """-> (FASTX text, records, slots): n reads with N / lowercase / U letters and awkward headers; reads without alignments; the alignments of
    key (0, 0) with the strands of STRAND_SETS, alignments of the other keys in the slots between them"""
    rng = np.random.Generator(np.random.PCG64(seed))
    text, recs = [], []
    for i in range(n):
        L = 5003 if (long_read and i == n // 2) else int(rng.integers(40, 160))
        seq = "".join("ACGTNacgtUun"[int(c)] for c in rng.choice(12, L, p=[.2, .2, .2, .2, .03, .03, .03, .03, .03, .03, .01, .01]))
        hdr = HEADERS[i % len(HEADERS)] % i
        qual = "".join(chr(33 + (7 * j + i) % 41) for j in range(L)) if i % 11 != 5 else ""
        text.append(("@%s\n%s\n+\n%s\n" % (hdr, seq, qual)) if fastq else (">%s\n%s\n" % (hdr, seq)))
        alns = []
        if i % 4 != 3 or L > 1000:                  # every fourth read has no alignment
            strands = STRAND_SETS[(i // 2) % len(STRAND_SETS)]
            for j, st in enumerate(strands):
                if i % 3 == 1 and len(alns) < slots - 1:       # another key's alignment in the slot in front: it neither appears nor counts
                    alns.append(craft_alignment(rng, L, ref_lens, KEYS[1 + (i + j) % 2], int(rng.integers(0, 2)), int(rng.integers(0, 4))))
                if len(alns) < slots:
                    alns.append(craft_alignment(rng, L, ref_lens, KEYS[0], st, (i + j) % 4, many_ops=L > 1000 or i % 13 == 0,
                                                score=60000 if (i, j) == (2, 0) else None))
        recs.append(record(alns, slots))
    return "".join(text).encode(), recs, slots


def open_report(tmpdir, fastq, cols, reg, dbs=DB, sam=True):
    os.makedirs(str(tmpdir), exist_ok=True)
    rep = report.Report(str(tmpdir), is_fastq=fastq, fastx=False, other=False, blast_cols=cols, sam=sam)
    for k, (lam, K, fr, fq) in dbs.items():
        rep.set_db(k, lam, K, fr, fq)
    for (k, part), ix in reg.items():
        rep.set_part(k, part, ix)
    return rep


def files(tmpdir, cols):
    sam = open(os.path.join(str(tmpdir), "aligned.sam"), "rb").read()
    blast = open(os.path.join(str(tmpdir), "aligned.blast"), "rb").read() if cols is not None else b""
    return sam, blast


def host_files(tmpdir, reads, recs, fastq, cols, reg, dbs=DB):
    """the per-read host loop: smr_reads_record_text + smr_report_add -> (aligned.sam, aligned.blast) as bytes"""
    rep = open_report(tmpdir, fastq, cols, reg, dbs)
    for i, rec in enumerate(recs):
        hdr, seq, qual = reads.record_text(i)
        rep.add(hdr, seq, qual, rec)
    rep.close()
    return files(tmpdir, cols)


def strip_header(sam):
    lines = sam.split(b"\n")
    k = 0
    while k < len(lines) and lines[k][:4] in (b"@HD\t", b"@SQ\t", b"@PG\t"):
        k += 1
    return b"\n".join(lines[k:])


def device_files(tmpdir, e, fastq, cols, reg, params_of, dbs=DB, slot_of=None, streams=None):
    """smr_rows_part per (index, part) + smr_report_add_rows, in a report that skips its own rows -> the two files; streams (a dict) gets the
    device's (sam, blast) per key"""
    rep = open_report(tmpdir, fastq, cols, reg, dbs)
    rep.skip_rows()
    for key, ix in reg.items():
        p = params_of(key)
        p.index_num, p.part = key
        slot = slot_of(key, ix) if slot_of else 0
        lam, K, fr, fq = dbs[key[0]]
        sam, blast = e.rows_part(slot, p, ix, sam=True, blast=cols is not None, cols=" ".join(cols or []), lam=lam, K=K, full_ref=fr, full_read=fq)
        if streams is not None:
            streams[key] = (sam, blast)
        rep.add_rows(key[0], key[1], sam, blast)
    rep.close()
    return files(tmpdir, cols)
