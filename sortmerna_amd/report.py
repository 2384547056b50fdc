"""ctypes wrapper of the report writers of libsmr_hip (smr_report_* in include/smr_hip.h): aligned/other FASTX, BLAST tabular, SAM
from the per-read records -- the reference's writeReports() pass (output.cpp:169-272)."""
import ctypes as C

import numpy as np

from . import capi
from .engine import OTU_GROUP, SmrError


def corrected_sizes(K, info, all_reads_count, all_reads_len, full_read_scale=1):
    """Refstats::full_ref / full_read after the length correction (refstats.cpp:238-257); full_read_scale: the number of processing threads of a
    reference run with -score_split (refstats.cpp:247), which the e-value of its BLAST report then carries too"""
    a, b = C.c_uint64(), C.c_uint64()
    capi.load().smr_refstats_corrected_split(K, info.bg, info.full_len, info.numseq, all_reads_count, all_reads_len, int(full_read_scale), C.byref(a), C.byref(b))
    return a.value, b.value


class Report:
    def __init__(self, out_dir, is_fastq, fastx=True, other=True, blast_cols=None, sam=False, blast_pairwise=False, sam_sq=False, cmdline=None,
                 paired_in=False, paired_out=False, out2=False, sout=False, zip_out=False, otu_map=False, denovo=False, min_id=0.0, min_cov=0.0):
        """blast_cols: None = no tabular BLAST report, else a list out of "cigar", "qcov", "qstrand" (output order);
        blast_pairwise: the `-blast 0` text instead; sam_sq: @SQ header lines (-SQ); cmdline: text of the SAM @PG CL: field;
        otu_map / denovo: otu_map.txt / aligned_denovo.fa|fq from records on which Engine.idcov_part ran with (min_id, min_cov); after close(),
        self.total_otu holds the number of groups written"""
        self.L = capi.load()
        o = capi.ReportOpts()
        o.fastx, o.other, o.sam = int(fastx), int(other), int(sam)
        o.blast_tabular = int(blast_cols is not None)
        o.blast_cols = " ".join(blast_cols or []).encode()
        o.blast_pairwise, o.sam_sq = int(blast_pairwise), int(sam_sq)
        o.paired_in, o.paired_out, o.out2, o.sout = int(paired_in), int(paired_out), int(out2), int(sout)
        o.zip_out = int(zip_out)
        o.otu_map, o.denovo, o.min_id, o.min_cov = int(otu_map), int(denovo), float(min_id), float(min_cov)
        self._otu = C.c_uint64(0)
        self.total_otu = 0
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = self.L.smr_report_open(out_dir.encode(), C.byref(o), int(is_fastq), C.byref(h), err, 512)
        if rc != 0:
            raise SmrError("smr_report_open: %s (rc=%d)" % (err.value.decode(), rc))
        self.h = h
        self._chk(self.L.smr_report_otu_count(self.h, C.byref(self._otu)), "smr_report_otu_count")
        if cmdline is not None:
            self._chk(self.L.smr_report_set_cmdline(self.h, cmdline.encode()), "smr_report_set_cmdline")

    def _chk(self, rc, what):
        if rc != 0:
            raise SmrError("%s: %s (rc=%d)" % (what, self.L.smr_report_last_error(self.h).decode(), rc))

    def set_db(self, index_num, lam, K, full_ref_corr, full_read_corr):
        self._chk(self.L.smr_report_set_db(self.h, index_num, lam, K, full_ref_corr, full_read_corr), "smr_report_set_db")

    def set_part(self, index_num, part, index):
        self._chk(self.L.smr_report_set_part(self.h, index_num, part, index.h), "smr_report_set_part")

    def add(self, header, seq, qual, record):
        self._chk(self.L.smr_report_add(self.h, header.encode(), seq.encode(), qual.encode() if qual else None, record, len(record)),
                  "smr_report_add")

    def add_pair(self, mate1, mate2):
        """mate = (header, seq, qual, record): routed like the reference's paired FASTX reports (-paired_in / -paired_out / -out2 / -sout)"""
        (h1, s1, q1, r1), (h2, s2, q2, r2) = mate1, mate2
        self._chk(self.L.smr_report_add_pair(self.h, h1.encode(), s1.encode(), q1.encode() if q1 else None, r1, len(r1),
                                             h2.encode(), s2.encode(), q2.encode() if q2 else None, r2, len(r2)), "smr_report_add_pair")

    def add_fastx(self, streams):
        """the eight streams of Engine.fastx_split (aligned[0..3], other[0..3]) appended to the open aligned.* / other.* files (smr_report_add_fastx)"""
        off = (C.c_uint64 * 9)()
        for k in range(8):
            off[k + 1] = off[k] + len(streams[k])
        blob = b"".join(streams)
        self._chk(self.L.smr_report_add_fastx(self.h, blob if blob else None, off), "smr_report_add_fastx")

    def skip_fastx(self, on=True):
        """add / add_pair leave aligned.* / other.* alone: add_fastx writes them (smr_report_skip_fastx)"""
        self._chk(self.L.smr_report_skip_fastx(self.h, int(bool(on))), "smr_report_skip_fastx")

    def add_rows(self, index_num, part, sam, blast):
        """the two streams of Engine.rows_part appended to the report's SAM / BLAST rows of (index_num, part) (smr_report_add_rows)"""
        off = (C.c_uint64 * 3)(0, len(sam), len(sam) + len(blast))
        blob = bytes(sam) + bytes(blast)
        self._chk(self.L.smr_report_add_rows(self.h, index_num, part, blob if blob else None, off), "smr_report_add_rows")

    def skip_rows(self, on=True):
        """add / add_pair leave SAM and BLAST tabular alone: add_rows brings them (smr_report_skip_rows)"""
        self._chk(self.L.smr_report_skip_rows(self.h, int(bool(on))), "smr_report_skip_rows")

    def add_pairwise(self, index_num, part, data):
        """the stream of Engine.pairwise_part appended to the report's BLAST pairwise text of (index_num, part) (smr_report_add_pairwise)"""
        data = bytes(data)
        self._chk(self.L.smr_report_add_pairwise(self.h, index_num, part, data if data else None, len(data)), "smr_report_add_pairwise")

    def skip_pairwise(self, on=True):
        """add / add_pair leave the BLAST pairwise text alone: add_pairwise brings it (smr_report_skip_pairwise)"""
        self._chk(self.L.smr_report_skip_pairwise(self.h, int(bool(on))), "smr_report_skip_pairwise")

    def add_otu(self, index_num, part, data, groups, any_yid_ycov):
        """the result of Engine.otu_part appended to the report's OTU map entries of (index_num, part) (smr_report_add_otu)"""
        data = bytes(data)
        g = np.ascontiguousarray(groups, dtype=OTU_GROUP)
        self._chk(self.L.smr_report_add_otu(self.h, index_num, part, data if data else None, len(data), g.ctypes.data if len(g) else None, len(g), int(bool(any_yid_ycov))),
                  "smr_report_add_otu")

    def skip_otu(self, on=True):
        """add / add_pair leave the OTU map alone: add_otu brings it (smr_report_skip_otu)"""
        self._chk(self.L.smr_report_skip_otu(self.h, int(bool(on))), "smr_report_skip_otu")

    def add_denovo(self, streams):
        """the four streams of Engine.fastx_denovo appended to the open aligned_denovo.* files (smr_report_add_denovo)"""
        off = (C.c_uint64 * 5)()
        for k in range(4):
            off[k + 1] = off[k] + len(streams[k])
        blob = b"".join(streams)
        self._chk(self.L.smr_report_add_denovo(self.h, blob if blob else None, off), "smr_report_add_denovo")

    def _add_gz(self, fn, streams, n):
        off = (C.c_uint64 * (n + 1))()
        for k in range(n):
            off[k + 1] = off[k] + len(streams[k])
        blob = b"".join(streams)
        self._chk(getattr(self.L, fn)(self.h, blob if blob else None, off), fn)

    def add_fastx_gz(self, streams):
        """the eight streams of Engine.fastx_split_gz -- gzip members -- appended as they are to the open aligned.* / other.* .gz files
        (smr_report_add_fastx_gz); the report must have been opened with zip_out"""
        self._add_gz("smr_report_add_fastx_gz", streams, 8)

    def add_denovo_gz(self, streams):
        """the four streams of Engine.fastx_denovo_gz appended as they are to the open aligned_denovo.* .gz files (smr_report_add_denovo_gz)"""
        self._add_gz("smr_report_add_denovo_gz", streams, 4)

    def add_rows_gz(self, index_num, part, sam_gz, blast_gz):
        """the two streams of Engine.rows_part_gz -- gzip members -- kept with the report's SAM / BLAST rows of (index_num, part) and written as
        they are at close (smr_report_add_rows_gz); the report must have been opened with zip_out"""
        off = (C.c_uint64 * 3)(0, len(sam_gz), len(sam_gz) + len(blast_gz))
        blob = bytes(sam_gz) + bytes(blast_gz)
        self._chk(self.L.smr_report_add_rows_gz(self.h, index_num, part, blob if blob else None, off), "smr_report_add_rows_gz")

    def add_pairwise_gz(self, index_num, part, gz):
        """the members of Engine.pairwise_part_gz kept with the report's BLAST pairwise text of (index_num, part) (smr_report_add_pairwise_gz)"""
        gz = bytes(gz)
        self._chk(self.L.smr_report_add_pairwise_gz(self.h, index_num, part, gz if gz else None, len(gz)), "smr_report_add_pairwise_gz")

    def skip_denovo(self, on=True):
        """add / add_pair leave aligned_denovo.* alone: add_denovo writes them (smr_report_skip_denovo)"""
        self._chk(self.L.smr_report_skip_denovo(self.h, int(bool(on))), "smr_report_skip_denovo")

    def merge_otu_from(self, other):
        """the OTU map entries of `other` (the next shard of the reads, in input order) behind this report's; `other` then writes no map"""
        self._chk(self.L.smr_report_otu_merge(self.h, other.h), "smr_report_otu_merge")

    def close(self):
        if self.h:
            rc = self.L.smr_report_close(self.h)
            self.h = None
            self.total_otu = int(self._otu.value)
            if rc != 0:
                raise SmrError("smr_report_close rc=%d" % rc)


def write_summary(path, dbs, reads_files, total_reads, num_aligned, all_reads_len, min_read_len, max_read_len, seed_len=18, num_seeds=2, edges=4,
                  match=2, mismatch=-3, gap_open=5, gap_ext=2, score_N=-3, sam_sq=False, threads=1, cmdline="", pid="", timestamp="",
                  total_denovo=None, total_id_cov=None, total_otu=0):
    """aligned.log (summary.cpp:102-175).  dbs: list of dicts {ref_file, skiplengths, lam, K, minimal_score, reads_matched}; total_denovo (-de_novo_otu) / total_id_cov + total_otu (-otu_map): the two
    optional Results lines, None = not printed"""
    L = capi.load()
    arr = (capi.SummaryDb * len(dbs))()
    for i, d in enumerate(dbs):
        arr[i].ref_file = d["ref_file"].encode()
        for k in range(3):
            arr[i].skiplengths[k] = d["skiplengths"][k]
        arr[i].lam, arr[i].K, arr[i].minimal_score, arr[i].reads_matched = d["lam"], d["K"], d["minimal_score"], d["reads_matched"]
    rf = (C.c_char_p * len(reads_files))(*[r.encode() for r in reads_files])
    s = capi.Summary()
    s.cmdline, s.pid, s.timestamp = cmdline.encode(), pid.encode(), timestamp.encode()
    s.seed_len, s.num_seeds, s.edges, s.match, s.mismatch, s.gap_open, s.gap_ext, s.score_N = seed_len, num_seeds, edges, match, mismatch, gap_open, gap_ext, score_N
    s.sam_sq, s.threads = int(sam_sq), threads
    s.reads_files, s.n_reads_files = rf, len(reads_files)
    s.total_reads, s.num_aligned, s.all_reads_len, s.min_read_len, s.max_read_len = total_reads, num_aligned, all_reads_len, min_read_len, max_read_len
    s.dbs, s.n_dbs = arr, len(dbs)
    s.is_denovo, s.total_denovo = int(total_denovo is not None), total_denovo or 0
    s.is_otu_map, s.total_id_cov, s.total_otu = int(total_id_cov is not None), total_id_cov or 0, total_otu
    rc = L.smr_summary_write(path.encode(), C.byref(s))
    if rc != 0:
        raise SmrError("smr_summary_write rc=%d" % rc)
