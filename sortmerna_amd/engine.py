"""Host-side mirror of the reference's alignment driver for the hot path.

`align()` below has the shape of processor.cpp:align() (/root/reference/src/sortmerna/processor.cpp:173-285):
for every index and every part: load index + references, run the per-read path over all reads, keep per-read
state between parts -- except that the inner N x align2() thread loop is one call into libsmr_hip (GPU).
"""
import ctypes as C

import numpy as np

from . import capi


# smr_otu_group of include/smr_hip.h
OTU_GROUP = np.dtype([("ref_num", np.uint32), ("n_reads", np.uint32), ("off", np.uint64)])


class SmrError(RuntimeError):
    pass


def default_params(**kw):
    p = capi.Params()
    capi.load().smr_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "skiplengths":
            for i in range(3):
                p.skiplengths[i] = v[i]
        else:
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
    return p


U64P = C.POINTER(C.c_uint64)


def _err_call(fn, *args):
    """fn(*args, err, 512) of the library, for the calls that say what went wrong in a buffer of the caller's; raises SmrError with that text"""
    err = C.create_string_buffer(512)
    rc = getattr(capi.load(), fn)(*args, err, 512)
    if rc != 0:
        raise SmrError("%s: %s (rc=%d)" % (fn, err.value.decode(), rc))


def _new_handle(cls, fn, *args):
    """cls(handle) of the object that fn(*args, &handle, err, 512) makes"""
    h = C.c_void_p()
    _err_call(fn, *args, C.byref(h))
    return cls(h)


def _packed(items):
    """(off, blob) of a list of byte strings (or of what bytes() takes): item i is blob[off[i]:off[i + 1]], off a uint64 array of len(items) + 1
    entries, blob a uint8 array of the items back to back and one NUL behind them (so that an empty list has an address as well)"""
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in items], dtype=np.uint64)
    return off, np.frombuffer(b"".join(bytes(x) for x in items) + b"\0", dtype=np.uint8)


class Index:
    """One (index, part) on the host: flattened lookup / mini-trie arena / positions CSR / reference bytes."""

    def __init__(self, handle):
        self.h = handle

    @staticmethod
    def load_files(prefix, part, ref_fasta):
        return _new_handle(Index, "smr_index_load_files", prefix.encode(), part, ref_fasta.encode())

    @staticmethod
    def _built(fn, *args):
        """-> list of Index: the parts that the builder fn(*args, handles, 256, &n, err, 512) leaves"""
        arr = (C.c_void_p * 256)()
        n = C.c_uint32()
        _err_call(fn, *args, C.cast(arr, C.POINTER(C.c_void_p)), 256, C.byref(n))
        return [Index(C.c_void_p(arr[i])) for i in range(n.value)]

    @staticmethod
    def build(ref_fasta, seed_win_len=18, max_file_size_mb=3072.0, max_pos=10000, threads=0):
        """-> list of Index (one per part)"""
        return Index._built("smr_index_build", ref_fasta.encode(), seed_win_len, max_file_size_mb, max_pos, threads)

    @staticmethod
    def build_gpu(engine, ref_fasta, seed_win_len=18, max_file_size_mb=3072.0, max_pos=10000):
        """like build(), with the sorting / id / position / mini-trie work on the device (smr_index_build_gpu)"""
        return Index._built("smr_index_build_gpu", engine.h, ref_fasta.encode(), seed_win_len, max_file_size_mb, max_pos)

    @staticmethod
    def write_files(parts, ref_fasta, prefix):
        arr = (C.c_void_p * len(parts))(*[p.h for p in parts])
        _err_call("smr_index_write_files", C.cast(arr, C.POINTER(C.c_void_p)), len(parts), ref_fasta.encode(), prefix.encode())

    def save(self, path, stamp=0):
        """flat cache of this part's host layout (smr_index_save)"""
        _err_call("smr_index_save", self.h, path.encode(), stamp)

    @staticmethod
    def load_flat(path, stamp=0):
        return _new_handle(Index, "smr_index_load_flat", path.encode(), stamp)

    def selfcheck(self):
        """the pigeonhole device layout holds the same entries, with their DFS ranks, as the reference-shaped one"""
        _err_call("smr_index_selfcheck", self.h)

    def info(self):
        i = capi.IndexInfo()
        capi.load().smr_index_get_info(self.h, C.byref(i))
        return i

    def free(self):
        if self.h:
            capi.load().smr_index_free(self.h)
            self.h = None


class Reads:
    def __init__(self, handle, keep=None):
        self.h = handle
        self._keep = keep          # the bytes a batch of Engine.upload_fastx(bytes) borrows its text from

    @staticmethod
    def from_seqs(seqs):
        offs, blob = _packed([s.encode("latin-1") for s in seqs])
        h = C.c_void_p()
        rc = capi.load().smr_reads_pack(blob.ctypes.data_as(C.c_char_p), offs.ctypes.data, len(seqs), C.byref(h))
        if rc != 0:
            raise SmrError("smr_reads_pack rc=%d" % rc)
        return Reads(h)

    @staticmethod
    def from_fastx(path, first=0, count=0):
        return _new_handle(Reads, "smr_reads_load_fastx", path.encode(), first, count)

    @staticmethod
    def from_fastx_mt(path, threads=0):
        """whole file, parsed and packed by `threads` threads (0 = all cores)"""
        return _new_handle(Reads, "smr_reads_load_fastx_mt", path.encode(), threads)

    @staticmethod
    def from_fastx_text(path, threads=0):
        """from_fastx_mt + the file text kept, so that record_text(i) returns (header line, letters, quality) for the report writers"""
        return _new_handle(Reads, "smr_reads_load_fastx_text", path.encode(), threads)

    def slice(self, first, count):
        """records [first, first+count) as a batch of their own (the read shard of one rank / one pipeline chunk)"""
        h = C.c_void_p()
        rc = capi.load().smr_reads_slice(self.h, first, count, C.byref(h))
        if rc != 0:
            raise SmrError("smr_reads_slice rc=%d" % rc)
        return Reads(h)

    @property
    def is_fastq(self):
        return bool(capi.load().smr_reads_is_fastq(self.h))

    def record_text(self, i):
        L = capi.load()
        lens = (C.c_size_t * 3)()
        rc = L.smr_reads_record_text(self.h, i, None, 0, None, 0, None, 0, lens)
        if rc != 0:
            raise SmrError("smr_reads_record_text rc=%d (batch not loaded with from_fastx_text?)" % rc)
        bufs = [C.create_string_buffer(lens[k] + 1) for k in range(3)]
        L.smr_reads_record_text(self.h, i, bufs[0], lens[0] + 1, bufs[1], lens[1] + 1, bufs[2], lens[2] + 1, lens)
        return tuple(b.value.decode() for b in bufs)

    @property
    def digest(self):
        return capi.load().smr_reads_digest(self.h)

    @property
    def count(self):
        return capi.load().smr_reads_count(self.h)

    @property
    def total_len(self):
        return capi.load().smr_reads_total_len(self.h)

    @property
    def min_len(self):
        return capi.load().smr_reads_min_len(self.h)

    @property
    def max_len(self):
        return capi.load().smr_reads_max_len(self.h)

    def free(self):
        if self.h:
            capi.load().smr_reads_free(self.h)
            self.h = None


def minimal_score(lam, K, info, all_reads_count, all_reads_len, evalue=1.0, full_read_scale=1):
    """Refstats arithmetic (refstats.cpp:238-265) from Gumbel (lambda, K) + DB statistics + GLOBAL read totals; full_read_scale = the
    reference's processing threads under -score_split (refstats.cpp:247), else 1."""
    return capi.load().smr_minimal_score_split(lam, K, info.bg, info.full_len, info.numseq, all_reads_count, all_reads_len, evalue, full_read_scale)


def pigeonhole_layout(index):
    """(pg uint32[], root3 uint32[]) of a host index as the host transform builds it (smr_index_pigeonhole: a test seam; views into the index)"""
    pg, r3 = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
    npg, nr3 = C.c_uint64(), C.c_uint64()
    _err_call("smr_index_pigeonhole", index.h, C.byref(pg), C.byref(npg), C.byref(r3), C.byref(nr3))
    return np.ctypeslib.as_array(pg, shape=(npg.value,)), np.ctypeslib.as_array(r3, shape=(nr3.value,))


ROUTE_RECORD, ROUTE_GATHER, ROUTE_CHAIN, ROUTE_EXT = 1, 2, 4, 8      # SMR_ROUTE_* of smr_hip.h (Engine.cand_routes)
FASTX_VIEW = 1                                                       # SMR_FASTX_VIEW (Engine.upload_fastx)
FASTX_KEEP = 2                                                       # SMR_FASTX_KEEP
FASTX_INFLATE = 4                                                    # SMR_FASTX_INFLATE
GUNZIP_WHY = ("", "not taken", "candidates", "rounds", "decode", "distance", "check", "truncated", "trailing", "header crc")      # smr_gunzip_info


class Engine:
    """One GPU.  Fails loudly when no HIP device / library is available (no CPU fallback)."""

    def __init__(self, device=0):
        self.L = capi.load()
        self.h = C.c_void_p()
        _err_call("smr_create", device, C.byref(self.h))
        self.n_reads = 0
        self._batch_n = {}
        self._cur = 0

    def _chk(self, rc, what):
        if rc != 0:
            raise SmrError("%s: %s (rc=%d)" % (what, self.L.smr_last_error(self.h).decode(), rc))

    def _fill(self, what, call, kinds=(np.uint8,), always=False):
        """The size-then-fill protocol of smr_hip.h for the call named `what` (as its SmrError names it).  `call(need, (buf, cap), ...)` makes it,
        with one (buffer, capacity) pair per entry of `kinds` -- (None, 0) for the sizes only -- and `need` the uint64 array, one entry per pair,
        that the library leaves the sizes in.  The call is made for the sizes, then once more with zeroed arrays of those sizes (of one element
        at least, so that each has an address) unless the last size is 0; -> the arrays, cut to the sizes (the array itself for one kind).
        What the callers differ in:
          * gunzip_batch, gunzip_tasks and seed_hits make the second call even for size 0 (always=True);
          * otu_part and otu_part_mates have two buffers, the text and the groups, and the number of groups decides whether to fetch;
          * export_state hands out the array as it is, so a batch without records gives a zero-length array;
          * gzip_batch and gzip_lines_batch do not come here: with a bound for the buffer their one call is enough (_gzip)."""
        need = (C.c_uint64 * len(kinds))()
        self._chk(call(need, *[(None, 0)] * len(kinds)), what)
        bufs = [np.zeros(max(n, 1), dtype=k) for n, k in zip(need, kinds)]
        if always or need[-1]:
            self._chk(call(need, *[(b.ctypes.data, n) for b, n in zip(bufs, list(need))]), what)
        out = [b[:n] for b, n in zip(bufs, need)]
        return out[0] if len(out) == 1 else out

    def upload_index(self, index, slot=0):
        self._chk(self.L.smr_index_upload(self.h, index.h, slot), "smr_index_upload")

    def check_device_index(self, index, slot=0):
        """the pigeonhole layout built on the device for `slot` == the host transform of the same index (raises SmrError on a difference)"""
        self._chk(self.L.smr_index_check_device(self.h, slot, index.h), "smr_index_check_device")

    def unload_index(self, slot=0):
        self._chk(self.L.smr_index_unload(self.h, slot), "smr_index_unload")

    def select_batch(self, batch):
        self._chk(self.L.smr_batch_select(self.h, batch), "smr_batch_select")
        self.n_reads = self._batch_n.get(batch, 0)
        self._cur = batch

    def set_seed_mode(self, exact_counters):
        """0: pigeonhole seed search (default); 1: per-lane DFS kernel with reference-exact work counters (same results)"""
        self._chk(self.L.smr_set_seed_mode(self.h, int(bool(exact_counters))), "smr_set_seed_mode")

    def sw_mode(self, set_to=-1):
        """Smith-Waterman kernel in use: 1 = packed 16-bit (default when the device self-check passes), 0 = 32-bit; set_to 0/1 selects"""
        return self.L.smr_sw_mode(self.h, set_to)

    def walk_rounds(self):
        """rounds of the candidate walk the next align_part runs, per pass (smr_walk_rounds)"""
        out = (C.c_uint32 * 3)()
        self._chk(self.L.smr_walk_rounds(self.h, out), "smr_walk_rounds")
        return list(out)

    def sw_selfcheck(self, n_cases=256, seed=1, max_len=700):
        """packed vs 32-bit Smith-Waterman kernel on n_cases random pairs x 2 scoring schemes, on the device; returns the number of differing cases"""
        bad = C.c_uint64()
        self._chk(self.L.smr_sw_selfcheck(self.h, n_cases, seed, max_len, C.byref(bad)), "smr_sw_selfcheck")
        return bad.value

    def ssw_batch(self, reads, refs, match=2, mismatch=-3, score_N=-3, gap_open=5, gap_ext=2, filters=0, mode=1):
        """reads / refs: lists of byte strings in the 0..4 alphabet; -> int32 array (n, 5): score1, ref_begin1, ref_end1, read_begin1, read_end1
        (ssw_align with flag 2, without the CIGAR), computed by the 32-bit (mode 0) or the packed (mode 1) SW kernel; mode 5: through the long-read strips"""
        n = len(reads)
        (ro, rb), (fo, fb) = _packed(reads), _packed(refs)
        out = np.zeros((n, 5), dtype=np.int32)
        self._chk(self.L.smr_ssw_batch(self.h, n, rb.ctypes.data, ro.ctypes.data, fb.ctypes.data, fo.ctypes.data, match, mismatch, score_N,
                                       gap_open, gap_ext, filters, mode, out.ctypes.data), "smr_ssw_batch")
        return out

    # one task of sw16_batch: smr_sw16_task of include/smr_hip.h
    SW16_TASK = np.dtype([("read", "<u4"), ("win_off", "<u4"), ("aq", "<u2"), ("m", "<u2"), ("nref", "<u2"), ("reversed", "u1"), ("list_b", "u1")])

    def sw16_batch(self, tasks, ref, rows, match=2, mismatch=-3, score_N=-3, gap_open=5, gap_ext=2, filters=0, blocks=0, force_any_n=False):
        """k_sw16<rows> over the reads of the selected batch (upload_reads) as the candidate walk launches it (smr_sw16_batch).  tasks: tuples
        (read, aq, m, reversed, win_off, nref, list_b); ref: bytes in the 0..4 alphabet that stand in for an index part's reference letters;
        -> int32 array (n, 5): score1, ref_begin1, ref_end1, read_begin1, read_end1 of the span against the window (list_b: the score, then -1)"""
        n = len(tasks)
        t = np.zeros(max(n, 1), dtype=self.SW16_TASK)
        for i, (r, aq, m, rev, wo, nref, lb) in enumerate(tasks):
            t[i] = (r, wo, aq, m, nref, rev, lb)
        rf = np.frombuffer(bytes(ref) + b"\0", dtype=np.uint8).copy()
        out = np.zeros((max(n, 1), 5), dtype=np.int32)
        self._chk(self.L.smr_sw16_batch(self.h, n, t.ctypes.data, rf.ctypes.data, len(ref), int(bool(force_any_n)), match, mismatch, score_N, gap_open, gap_ext,
                                        filters, rows, blocks, out.ctypes.data), "smr_sw16_batch")
        return out[:n]

    SW16_PREFIX_TASK = np.dtype([("read", "<u4"), ("win_off", "<u4"), ("aq", "<u2"), ("m", "<u2"), ("nref", "<u2"), ("cols", "<u2"), ("reversed", "u1"), ("pad_", "V3")])

    def sw16_prefix_batch(self, tasks, ref, rows, match=2, mismatch=-3, score_N=-3, gap_open=5, gap_ext=2, blocks=0, force_any_n=False, **_):
        """the prefix tasks of k_sw16<rows> (smr_sw16_prefix_batch).  tasks: tuples (read, aq, m, reversed, win_off, nref, cols);
        -> int32 array (n, 2): lo, hi -- the interval that holds the score of the span against the whole window, from its first cols columns"""
        n = len(tasks)
        t = np.zeros(max(n, 1), dtype=self.SW16_PREFIX_TASK)
        for i, (r, aq, m, rev, wo, nref, cols) in enumerate(tasks):
            t[i] = (r, wo, aq, m, nref, cols, rev, b"")
        rf = np.frombuffer(bytes(ref) + b"\0", dtype=np.uint8).copy()
        out = np.zeros((max(n, 1), 2), dtype=np.int32)
        self._chk(self.L.smr_sw16_prefix_batch(self.h, n, t.ctypes.data, rf.ctypes.data, len(ref), int(bool(force_any_n)), match, mismatch, score_N, gap_open, gap_ext,
                                               rows, blocks, out.ctypes.data), "smr_sw16_prefix_batch")
        return out[:n]

    def walk_prefix_stats(self):
        """prefix tasks of the candidate walk since prof_reset (smr_walk_prefix_stats): scored, decided, redone, unused; the look-ahead tasks of reads
        expected to align under best N and their cells; percent = SMR_WALK_PREFIX as latched"""
        out = (C.c_uint64 * 8)()
        self._chk(self.L.smr_walk_prefix_stats(self.h, out), "smr_walk_prefix_stats")
        return dict(zip(("scored", "decided", "redone", "unused", "ahead", "ahead_cells", "percent", "live"), out[:8]))

    def sw16_launches(self):
        """launches of k_sw16<13 | 19 | 26 | 32> since the engine was created: ({rows: by the walk rounds}, {rows: by the begin-cell stage})"""
        out = (C.c_uint64 * 8)()
        self._chk(self.L.smr_sw16_launches(self.h, out), "smr_sw16_launches")
        return dict(zip((13, 19, 26, 32), out[:4])), dict(zip((13, 19, 26, 32), out[4:]))

    def sw16_f16(self, set_to=-1):
        """k_sw16h, the packed-f16 flavour of k_sw16, where the scoring scheme allows it (smr_sw16_f16): set_to 0 / 1 selects, anything else only
        queries; -> (the mode in use, launches of k_sw16h since the engine was created)"""
        n = C.c_uint64(0)
        mode = self.L.smr_sw16_f16(self.h, int(set_to), C.byref(n))
        if mode < 0:
            self._chk(mode, "smr_sw16_f16")
        return mode, int(n.value)

    def sw_long_rows(self, m):
        """the strip height (8, 10 ... 24) the long-read Smith-Waterman scores a span of m rows with (smr_sw_long_rows)"""
        return self.L.smr_sw_long_rows(int(m))

    def cigar_batch(self, reads, refs, scores, match=2, mismatch=-3, score_N=-3, gap_open=5, gap_ext=2):
        """reads / refs: the aligned spans (byte strings in the 0..4 alphabet), scores: their score1; -> list of u32 CIGAR arrays (len << 4 | op),
        what the reference's banded_sw returns for each triple (the traceback kernels behind smr_traceback)"""
        n = len(reads)
        (ro, rb), (fo, fb) = _packed(reads), _packed(refs)
        sc = np.asarray(scores, dtype=np.uint16)
        off = np.zeros(n + 1, dtype=np.uint64)
        cap = int(ro[-1] + fo[-1]) + 4 * n + 16
        out = np.zeros(cap, dtype=np.uint32)
        self._chk(self.L.smr_cigar_batch(self.h, n, rb.ctypes.data, ro.ctypes.data, fb.ctypes.data, fo.ctypes.data, sc.ctypes.data, match, mismatch, score_N,
                                         gap_open, gap_ext, out.ctypes.data, cap, off.ctypes.data), "smr_cigar_batch")
        return [out[int(off[i]):int(off[i + 1])].copy() for i in range(n)]

    def upload_reads(self, reads, max_alignments_per_read=1):
        self._chk(self.L.smr_reads_upload(self.h, reads.h, max_alignments_per_read), "smr_reads_upload")
        self.n_reads = reads.count
        self._batch_n[self._cur] = reads.count

    def upload_reads_batch(self, batch, reads, max_alignments_per_read=1):
        """smr_reads_upload_batch: into batch `batch` without selecting it, on the context's upload stream (may run on a second host thread
        while the selected batch is being aligned)"""
        self._chk(self.L.smr_reads_upload_batch(self.h, batch, reads.h, max_alignments_per_read), "smr_reads_upload_batch")
        self._batch_n[batch] = reads.count

    def upload_fastx(self, data_or_path, max_alignments_per_read=1, batch=None, view=False, keep=False, inflate=False):
        """smr_reads_upload_fastx*: FASTA/FASTQ text (bytes), or the file at a path (str; gzip is inflated), parsed and 2-bit packed on the device
        into the selected batch -- or, with batch=k, into batch k on the upload stream.  Returns the Reads the host parser would have made of
        the same bytes, copied back from the device; view=True leaves the packed words there (SMR_FASTX_VIEW: record_text and the statistics
        work, digest is 0, slice and upload raise).  keep=True leaves the text with the batch on the device (SMR_FASTX_KEEP: the text plus 16 bytes
        per record of device memory) for fastx_split.  inflate=True: a gzip file (or gzip bytes) is inflated on the device (SMR_FASTX_INFLATE)."""
        h = C.c_void_p()
        flags = (FASTX_VIEW if view else 0) | (FASTX_KEEP if keep else 0) | (FASTX_INFLATE if inflate else 0)
        keep = None
        if isinstance(data_or_path, str):
            if batch is not None:
                raise SmrError("upload_fastx: batch= takes bytes (read the file first)")
            err = C.create_string_buffer(512)
            rc, what = self.L.smr_reads_upload_fastx_file(self.h, data_or_path.encode(), max_alignments_per_read, flags, C.byref(h), err, 512), "smr_reads_upload_fastx_file"
        else:
            keep = C.create_string_buffer(bytes(data_or_path), len(data_or_path) + 1)          # (the Reads borrows these bytes)
            if batch is None:
                rc, what = self.L.smr_reads_upload_fastx(self.h, keep, len(data_or_path), max_alignments_per_read, flags, C.byref(h)), "smr_reads_upload_fastx"
            else:
                rc, what = self.L.smr_reads_upload_fastx_batch(self.h, batch, keep, len(data_or_path), max_alignments_per_read, flags, C.byref(h)), "smr_reads_upload_fastx_batch"
        self._chk(rc, what)
        reads = Reads(h, keep)
        if batch is None:
            self.n_reads = reads.count
        self._batch_n[self._cur if batch is None else batch] = reads.count
        return reads

    def fastx_info(self):
        """(path taken: 0 the kernels, 1 the host parser; lines found; records; text bytes uploaded) of the last upload_fastx (smr_fastx_info: a test seam)"""
        info = (C.c_uint64 * 4)()
        self._chk(self.L.smr_fastx_info(self.h, info), "smr_fastx_info")
        return tuple(int(x) for x in info)

    def _times(self, fn, names):
        """the HIP-event ms that the smr_*_times call `fn` reports, one per name -> dict"""
        ms = (C.c_double * len(names))()
        self._chk(getattr(self.L, fn)(self.h, ms), fn)
        return dict(zip(names, (float(x) for x in ms)))

    def fastx_times(self):
        """HIP-event ms of the last upload_fastx on the device path: dict(h2d, lines, records, pack, d2h)"""
        return self._times("smr_fastx_times", ("h2d", "lines", "records", "pack", "d2h"))

    def fastx_split(self, layout=0, mates=None, paired_in=False, paired_out=False, out2=False, sout=False, aligned=True, other=True, hit=None):
        """smr_fastx_split: the aligned.* / other.* FASTX streams of the selected batch (uploaded with keep=True), written on the device -> a list
        of eight bytes objects, aligned[0..3] then other[0..3].  layout 0: single reads; 1: mates interleaved; 2: the mates are the reads of batch
        `mates`.  hit: one truth value per read (the selected batch's, then the mates') used instead of the batch's own is_hit."""
        return self._fx("smr_fastx_split", 8, self._fx_opts(layout, paired_in, paired_out, out2, sout, aligned, other), hit, mates)[0]

    def fastx_split_times(self):
        """HIP-event ms of the last fastx_split: dict(measure, scans, copy, d2h)"""
        return self._times("smr_fastx_split_times", ("measure", "scans", "copy", "d2h"))

    def rows_part(self, slot, params, index, sam=True, blast=False, cols="", lam=0.0, K=0.0, full_ref=0, full_read=0):
        """smr_rows_part: the rows of aligned.sam and of the BLAST tabular report of the selected batch (uploaded with keep=True) for the
        (index, part) of `params`, resident in `slot`, written on the device -> (sam_bytes, blast_bytes).  cols: "cigar", "qcov", "qstrand",
        space separated or as a list, in output order; lam, K, full_ref, full_read: what Report.set_db takes for that index."""
        return self._rows("smr_rows_part", None, slot, params, index, sam, blast, cols, lam, K, full_ref, full_read)

    def rows_times(self):
        """HIP-event ms of the last rows_part: dict(stats, sizes, write, d2h)"""
        return self._times("smr_rows_times", ("stats", "sizes", "write", "d2h"))

    def pairwise_part(self, slot, params, index, lam=0.0, K=0.0, full_ref=0, full_read=0):
        """smr_pairwise_part: the BLAST-like pairwise text (-blast 0) of the selected batch (uploaded with keep=True) for the (index, part) of
        `params`, resident in `slot`, written on the device -> bytes.  lam, K, full_ref, full_read: what Report.set_db takes for that index."""
        return self._pairwise("smr_pairwise_part", None, slot, params, index, lam, K, full_ref, full_read)

    def pairwise_times(self):
        """HIP-event ms of the last pairwise_part: dict(stats, sizes, write, d2h)"""
        return self._times("smr_pairwise_times", ("stats", "sizes", "write", "d2h"))

    def otu_part(self, slot, params, index, min_id, min_cov):
        """smr_otu_part: the members of otu_map.txt of the selected batch (uploaded with keep=True, after idcov_part of every part) for the
        (index, part) of `params`, resident in `slot`, grouped and written on the device -> (bytes, groups, any): groups is a structured array
        (ref_num, n_reads, off), ascending in ref_num; the text of group g is bytes[off[g]:off[g + 1]] (the last: to the end), its ids joined
        by tabs; any: does a read of the batch have c_yid_ycov > 0 (is there a map file at all)"""
        return self._otu("smr_otu_part", None, slot, params, index, min_id, min_cov)

    def otu_times(self):
        """HIP-event ms of the last otu_part: dict(classify, sizes, sort, write, d2h)"""
        return self._times("smr_otu_times", ("classify", "sizes", "sort", "write", "d2h"))

    def otu_part_mates(self, mates, slot, params, index, min_id, min_cov):
        """smr_otu_part_mates: otu_part for mates read from two files -- read i of the selected batch is mate 1 of pair i, read i of batch
        `mates` its mate 2; both uploaded with keep=True, idcov_part of every part run on both -> (bytes, groups, any) as otu_part gives them,
        the members of a group in pair order, mate 1 before mate 2; any: does a read of either batch have c_yid_ycov > 0"""
        return self._otu("smr_otu_part_mates", int(mates), slot, params, index, min_id, min_cov)

    def otu_mates_times(self):
        """HIP-event ms of the last otu_part_mates: dict(classify_a, sizes_a, classify_b, sizes_b, compact); otu_times gives the whole call"""
        return self._times("smr_otu_mates_times", ("classify_a", "sizes_a", "classify_b", "sizes_b", "compact"))

    def otu_sort_batch(self, keys, key_bits):
        """smr_otu_sort_batch (a test seam): the stable permutation that sorts keys (each below 2 ** key_bits) ascending, found by the radix
        sort of otu_part -> uint32 array"""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        perm = np.zeros(max(len(keys), 1), dtype=np.uint32)
        self._chk(self.L.smr_otu_sort_batch(self.h, len(keys), keys.ctypes.data if len(keys) else None, int(key_bits), perm.ctypes.data), "smr_otu_sort_batch")
        return perm[:len(keys)]

    @staticmethod
    def _denovo_opts(opts, kw):
        """a capi.FxSplitOpts as it is, or one made of a dict / keywords out of layout, paired_in, paired_out, out2, sout"""
        if isinstance(opts, capi.FxSplitOpts):
            return opts
        d = dict(opts or {}, **kw)
        return Engine._fx_opts(d.get("layout", 0), d.get("paired_in"), d.get("paired_out"), d.get("out2"), d.get("sout"), 1, 0)

    @staticmethod
    def _fx_opts(layout, paired_in, paired_out, out2, sout, aligned, other):
        return capi.FxSplitOpts(int(layout), int(bool(paired_in)), int(bool(paired_out)), int(bool(out2)), int(bool(sout)), int(bool(aligned)), int(bool(other)))

    def _fx(self, fn, n, o, flags, mates):
        """the n FASTX streams of smr_fastx_split / smr_fastx_denovo or of their _gz forms (fn) -> (a list of n bytes objects, the n + 1 offsets
        of the plain streams).  flags: one truth value per read to use instead of the batch's own, or None"""
        fb = None if flags is None else (C.c_uint8 * max(len(flags), 1))(*[1 if x else 0 for x in flags])
        return self._streams(fn, n, (self.h, -1 if mates is None else int(mates), C.byref(o), fb))

    def _streams(self, fn, n, head):
        """n streams in one buffer from the writer fn(*head, buf, cap, off, need) -- a _gz form: fn(*head, buf, cap, gz_off, plain_off, need) --
        -> (a list of n bytes objects, the n + 1 offsets the plain streams have)"""
        off, gz_off = (C.c_uint64 * (n + 1))(), (C.c_uint64 * (n + 1))()
        tail, cut = ((gz_off, off), gz_off) if fn.endswith("_gz") else ((off,), off)
        raw = self._fill(fn, lambda need, b: getattr(self.L, fn)(*head, *b, *tail, need)).tobytes()
        return [raw[cut[k]:cut[k + 1]] for k in range(n)], [int(x) for x in off]

    def _part_head(self, mates, slot, params, index):
        """the leading arguments of a writer of one (index, part): the plain call's, or with `mates` (a batch number) those of its _mates form"""
        return (self.h,) + (() if mates is None else (mates,)) + (slot, C.byref(params), index.h)

    def fastx_denovo(self, opts=None, mates=-1, dn=None, **kw):
        """smr_fastx_denovo: the aligned_denovo.* FASTX streams of the selected batch (uploaded with keep=True), written on the device -> a list
        of four bytes objects.  opts: a capi.FxSplitOpts, or a dict / keywords out of layout, paired_in, paired_out, out2, sout as fastx_split
        takes them (want_aligned / want_other are ignored); mates: the batch of the mates under layout 2, else -1.  dn: one truth value per
        read (the selected batch's, then the mates') used instead of the counters idcov_part left"""
        return self._fx("smr_fastx_denovo", 4, self._denovo_opts(opts, kw), dn, mates)[0]

    def gzip_chunk(self):
        """smr_gzip_chunk: plain bytes per gzip member of the device compressor"""
        return int(self.L.smr_gzip_chunk())

    def gzip_bound(self, plain_bytes, n_chunks):
        """smr_gzip_bound: no output of the device compressor for plain_bytes in n_chunks members is larger"""
        return int(self.L.smr_gzip_bound(int(plain_bytes), int(n_chunks)))

    def gzip_batch(self, streams):
        """smr_gzip_batch: every bytes object of `streams` cut into chunks of gzip_chunk() bytes and each chunk made a gzip member by the
        DEFLATE kernels -> a list of bytes objects, the members of each stream back to back (b"" for an empty one)"""
        chunk = self.gzip_chunk()
        return self._gzip("smr_gzip_batch", streams, self.gzip_bound(sum(len(x) for x in streams), sum((len(x) + chunk - 1) // chunk for x in streams)))

    def _gzip(self, fn, streams, cap):
        """smr_gzip_batch / smr_gzip_lines_batch (fn) over a list of bytes objects: one call into a buffer of `cap` bytes, their bound"""
        n = len(streams)
        off, plain = _packed(streams)
        gz_off = (C.c_uint64 * (n + 1))()
        need = C.c_uint64(0)
        buf = np.zeros(max(cap, 1), dtype=np.uint8)
        self._chk(getattr(self.L, fn)(self.h, plain.ctypes.data, off.ctypes.data_as(U64P), n, buf.ctypes.data, cap, gz_off, C.byref(need)), fn)
        raw = buf[:need.value].tobytes()
        return [raw[gz_off[k]:gz_off[k + 1]] for k in range(n)]

    def gunzip_batch(self, blob, grain=0):
        """smr_gunzip_batch: the gzip file `blob` (bytes, any number of members) inflated by the DEFLATE decoder kernels -> bytes.  grain: the
        least distance of two tasks in compressed bytes (0: the default, 1: a task at every candidate).  What the device does not settle is
        inflated by zlib inside the call (gunzip_info says which); a file zlib refuses raises SmrError."""
        gz = np.frombuffer(bytes(blob) or b"\0", dtype=np.uint8)
        return self._fill("smr_gunzip_batch", lambda need, b: self.L.smr_gunzip_batch(self.h, gz.ctypes.data, len(blob), int(grain), *b, need), always=True).tobytes()

    def gunzip_info(self):
        """smr_gunzip_info of the last gunzip_batch / inflating upload_fastx: dict(path "device" | "host", why (a word of GUNZIP_WHY), rounds,
        candidates, tasks, members, stored, fixed, dynamic (blocks), compressed, plain (bytes))"""
        info = (C.c_uint64 * 8)()
        self._chk(self.L.smr_gunzip_info(self.h, info), "smr_gunzip_info")
        v = [int(x) for x in info]
        return dict(path="host" if v[0] & 0xFF else "device", why=GUNZIP_WHY[(v[0] >> 8) & 0xFF], rounds=v[0] >> 16, candidates=v[1], tasks=v[2], members=v[3],
                    stored=v[4] & 0xFFFFFFFF, fixed=v[4] >> 32, dynamic=v[5], compressed=v[6], plain=v[7])

    def gunzip_times(self):
        """HIP-event ms of the last gunzip_batch / inflating upload_fastx on the device path: dict(h2d, find, count, write, window, resolve)"""
        return self._times("smr_gunzip_times", ("h2d", "find", "count", "write", "window", "resolve"))

    def gunzip_tasks(self):
        """smr_gunzip_tasks (a test seam): the confirmed tasks of the last call on the device path -> [(start bit, at a member header, made by the stitch)]"""
        tasks = self._fill("smr_gunzip_tasks", lambda n, b: self.L.smr_gunzip_tasks(self.h, C.cast(b[0], U64P), b[1], n), kinds=(np.uint64,), always=True)
        return [(int(x) >> 2, bool(x & 1), bool(x & 2)) for x in tasks.tolist()]

    def gzip_times(self):
        """HIP-event ms of the last gzip_batch / fastx_split_gz / fastx_denovo_gz: dict(match, codes, encode, compact, d2h)"""
        return self._times("smr_gzip_times", ("match", "codes", "encode", "compact", "d2h"))

    def fastx_split_gz(self, layout=0, mates=None, paired_in=False, paired_out=False, out2=False, sout=False, aligned=True, other=True, hit=None):
        """smr_fastx_split_gz: the eight streams of fastx_split, compressed on the device -> (a list of eight bytes objects, each the gzip
        members of its stream or b"", and the nine offsets fastx_split's streams would have)"""
        return self._fx("smr_fastx_split_gz", 8, self._fx_opts(layout, paired_in, paired_out, out2, sout, aligned, other), hit, mates)

    def fastx_denovo_gz(self, opts=None, mates=-1, dn=None, **kw):
        """smr_fastx_denovo_gz: the four streams of fastx_denovo, compressed on the device -> (four bytes objects, the five plain offsets)"""
        return self._fx("smr_fastx_denovo_gz", 4, self._denovo_opts(opts, kw), dn, mates)

    def gzip_lines_bound(self, plain_bytes, n_streams):
        """smr_gzip_lines_bound: no output of gzip_lines_batch / rows_part_gz / pairwise_part_gz for plain_bytes in n_streams streams is larger"""
        return int(self.L.smr_gzip_lines_bound(int(plain_bytes), int(n_streams)))

    def gzip_lines_batch(self, streams):
        """smr_gzip_lines_batch: gzip_batch with the members cut at line ends -- nominal cuts every 48 KiB, each moved back to behind the last
        newline of the 16 KiB in front of it -> a list of bytes objects, the members of each stream back to back (b"" for an empty one)"""
        return self._gzip("smr_gzip_lines_batch", streams, self.gzip_lines_bound(sum(len(x) for x in streams), len(streams)))

    def rows_part_gz(self, slot, params, index, sam=True, blast=False, cols="", lam=0.0, K=0.0, full_ref=0, full_read=0):
        """smr_rows_part_gz: the two streams of rows_part, compressed on the device into gzip members that end at line ends ->
        (sam_gz, blast_gz, plain_off): the members of each stream (b"" for one that is not wanted or holds no row) and the three offsets
        rows_part's streams would have.  Arguments as rows_part."""
        return self._rows("smr_rows_part_gz", None, slot, params, index, sam, blast, cols, lam, K, full_ref, full_read)

    def pairwise_part_gz(self, slot, params, index, lam=0.0, K=0.0, full_ref=0, full_read=0):
        """smr_pairwise_part_gz: the text of pairwise_part, compressed on the device into gzip members that end at line ends ->
        (gz, plain_bytes): the members and the size pairwise_part's text would have.  Arguments as pairwise_part."""
        return self._pairwise("smr_pairwise_part_gz", None, slot, params, index, lam, K, full_ref, full_read)

    @staticmethod
    def _rows_opts(sam, blast, cols, lam, K, full_ref, full_read):
        o = capi.RowsOpts()
        o.want_sam, o.want_blast = int(bool(sam)), int(bool(blast))
        o.blast_cols = (cols if isinstance(cols, str) else " ".join(cols)).encode()
        o.lam, o.K, o.full_ref_corr, o.full_read_corr = float(lam), float(K), int(full_ref), int(full_read)
        return o

    def _rows(self, fn, mates, slot, params, index, *opts):
        """smr_rows_part, its _mates and _gz forms (fn; mates: the batch of the mates, or None) -> (sam, blast), a _gz form: (sam, blast, plain offsets)"""
        o = self._rows_opts(*opts)
        (sam, blast), plain_off = self._streams(fn, 2, self._part_head(mates, slot, params, index) + (C.byref(o),))
        return (sam, blast, plain_off) if fn.endswith("_gz") else (sam, blast)

    def _pairwise(self, fn, mates, slot, params, index, lam, K, full_ref, full_read):
        """smr_pairwise_part, its _mates and _gz forms (fn; mates as for _rows) -> the text, a _gz form: (the gzip members, the size of the plain text)"""
        plain = C.c_uint64(0)
        head = self._part_head(mates, slot, params, index) + (float(lam), float(K), int(full_ref), int(full_read))
        tail = (C.byref(plain),) if fn.endswith("_gz") else ()
        text = self._fill(fn, lambda need, b: getattr(self.L, fn)(*head, *b, *tail, need)).tobytes()
        return (text, int(plain.value)) if tail else text

    def _otu(self, fn, mates, slot, params, index, min_id, min_cov):
        """smr_otu_part or its _mates form (fn; mates as for _rows) -> (bytes, groups, any)"""
        any_ = C.c_int(0)
        head = self._part_head(mates, slot, params, index) + (float(min_id), float(min_cov))
        text, groups = self._fill(fn, lambda need, b, g: getattr(self.L, fn)(*head, *b, *g, need, C.byref(any_)), kinds=(np.uint8, OTU_GROUP))
        return text.tobytes(), groups, bool(any_.value)

    def rows_part_mates(self, mates, slot, params, index, sam=True, blast=False, cols="", lam=0.0, K=0.0, full_ref=0, full_read=0):
        """smr_rows_part_mates: rows_part for mates in two reads files -- read i of the selected batch and read i of batch `mates` (both uploaded
        with keep=True) -- in the order in which Report.add_pair appends them -> (sam_bytes, blast_bytes).  Other arguments as rows_part."""
        return self._rows("smr_rows_part_mates", int(mates), slot, params, index, sam, blast, cols, lam, K, full_ref, full_read)

    def pairwise_part_mates(self, mates, slot, params, index, lam=0.0, K=0.0, full_ref=0, full_read=0):
        """smr_pairwise_part_mates: pairwise_part for mates in two reads files (the selected batch and batch `mates`), in the order of
        Report.add_pair -> bytes.  Other arguments as pairwise_part."""
        return self._pairwise("smr_pairwise_part_mates", int(mates), slot, params, index, lam, K, full_ref, full_read)

    def rows_part_mates_gz(self, mates, slot, params, index, sam=True, blast=False, cols="", lam=0.0, K=0.0, full_ref=0, full_read=0):
        """smr_rows_part_mates_gz: the two streams of rows_part_mates, compressed on the device -> (sam_gz, blast_gz, plain_off) as rows_part_gz"""
        return self._rows("smr_rows_part_mates_gz", int(mates), slot, params, index, sam, blast, cols, lam, K, full_ref, full_read)

    def pairwise_part_mates_gz(self, mates, slot, params, index, lam=0.0, K=0.0, full_ref=0, full_read=0):
        """smr_pairwise_part_mates_gz: the text of pairwise_part_mates, compressed on the device -> (gz, plain_bytes) as pairwise_part_gz"""
        return self._pairwise("smr_pairwise_part_mates_gz", int(mates), slot, params, index, lam, K, full_ref, full_read)

    def interleave_batch(self, a_pieces, b_pieces):
        """smr_interleave_batch (the seam of the interleave kernel): two equally long lists of bytes objects -> a[0] + b[0] + a[1] + b[1] + ..."""
        n = len(a_pieces)
        if len(b_pieces) != n:
            raise SmrError("interleave_batch: %d pieces against %d" % (n, len(b_pieces)))
        (a_off, a), (b_off, b) = _packed(a_pieces), _packed(b_pieces)
        args = (self.h, n, a.ctypes.data, a_off.ctypes.data_as(U64P), b.ctypes.data, b_off.ctypes.data_as(U64P))
        return self._fill("smr_interleave_batch", lambda need, out: self.L.smr_interleave_batch(*args, *out, need)).tobytes()

    def mates_times(self):
        """HIP-event ms of the last *_mates call: dict(selected, mates, interleave, d2h)"""
        return self._times("smr_mates_times", ("selected", "mates", "interleave", "d2h"))

    def rows_fmt_batch(self, num, den):
        """smr_rows_fmt_batch (a test seam): the device's `%.3g` of 100 * num[i] / den[i] -> list of str"""
        num = np.ascontiguousarray(num, dtype=np.uint32)
        den = np.ascontiguousarray(den, dtype=np.uint32)
        out = np.zeros((len(num), 16), dtype=np.uint8)
        self._chk(self.L.smr_rows_fmt_batch(self.h, len(num), num.ctypes.data, den.ctypes.data, out.ctypes.data), "smr_rows_fmt_batch")
        return [bytes(r).rstrip(b"\0").decode() for r in out] if len(num) < 4096 else out.view("S16").ravel().astype(str).tolist()

    def reset_state(self):
        self._chk(self.L.smr_state_reset(self.h), "smr_state_reset")

    def import_state(self, records):
        """the inverse of records(): one byte string per read of the selected batch, b"" = no stored record (smr_state_import), or the
        (blob, off) pair that export_state() returns.  The batch then continues as if this engine had produced that state itself"""
        if isinstance(records, tuple):
            blob, off = records
            blob = np.ascontiguousarray(blob, dtype=np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
            if blob.size == 0:
                blob = np.zeros(1, dtype=np.uint8)
            self._chk(self.L.smr_state_import(self.h, blob.ctypes.data, off.ctypes.data, len(off) - 1), "smr_state_import")
            return
        off, blob = _packed(records)
        self._chk(self.L.smr_state_import(self.h, blob.ctypes.data, off.ctypes.data, len(records)), "smr_state_import")

    def export_state(self):
        """the records of the selected batch, sized and serialised on the device (smr_state_export; no fetch() needed): -> (blob, off), record i
        is blob[off[i]:off[i + 1]], empty for a read without alignments.  What import_state takes and a state file holds"""
        n = self.n_reads
        off = np.zeros(n + 1, dtype=np.uint64)
        return self._fill("smr_state_export", lambda need, b: self.L.smr_state_export(self.h, *b, off.ctypes.data, n, need)), off

    def export_records(self):
        """export_state() cut into one byte string per read: what fetch() + records() give"""
        blob, off = self.export_state()
        raw = blob.tobytes()
        return [raw[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]

    def import_counters(self, values, n_db):
        """the inverse of counters(n_db): the dict it returns, or the flat sequence num_aligned, num_short, reads_matched_per_db[0..n_db)"""
        if isinstance(values, dict):
            values = [values["num_aligned"], values["num_short"]] + list(values["reads_matched_per_db"])
        if len(values) != 2 + n_db:
            raise SmrError("import_counters: %d values for n_db = %d (expected %d)" % (len(values), n_db, 2 + n_db))
        arr = (C.c_uint64 * (2 + n_db))(*[int(v) for v in values])
        self._chk(self.L.smr_counters_import(self.h, arr, n_db), "smr_counters_import")

    def align_part(self, slot, params):
        self._chk(self.L.smr_align_part(self.h, slot, C.byref(params)), "smr_align_part")

    def traceback(self, slot, params):
        self._chk(self.L.smr_traceback(self.h, slot, C.byref(params)), "smr_traceback")

    def idcov_part(self, slot, params, min_id, min_cov):
        """the %id / %coverage pass (the reference's denovo_stats) over the stored alignments of (params.index_num, params.part), whose references
        are resident in `slot`; after traceback() of every part of the run (smr_idcov_part)"""
        self._chk(self.L.smr_idcov_part(self.h, slot, C.byref(params), float(min_id), float(min_cov)), "smr_idcov_part")

    def idcov_counters(self):
        out = (C.c_uint64 * 4)()
        self._chk(self.L.smr_idcov_counters(self.h, out), "smr_idcov_counters")
        return dict(n_yid_ycov=out[0], n_yid_ncov=out[1], n_nid_ycov=out[2], num_denovo=out[3])

    def idcov_counters_device(self):
        p = C.c_void_p()
        n = C.c_uint32()
        self._chk(self.L.smr_idcov_counters_device(self.h, C.byref(p), C.byref(n)), "smr_idcov_counters_device")
        return p.value, n.value

    def idcov_batch(self, reads, refs, cigars, read_begin, read_end, readlen, min_id, min_cov):
        """reads: whole FORWARD reads, refs: the reference windows from each alignment's first reference letter on (byte strings in the 0..4
        alphabet), cigars: u32 arrays (len << 4 | op); -> uint32 array (n, 4): n_miss, n_gap, n_match, class 0..3 (smr_idcov_batch)"""
        n = len(reads)
        (ro, rb), (fo, fb) = _packed(reads), _packed(refs)
        co = np.zeros(n + 1, dtype=np.uint64)
        co[1:] = np.cumsum([len(x) for x in cigars])
        cg = np.concatenate([np.asarray(x, dtype=np.uint32) for x in cigars] + [np.zeros(1, dtype=np.uint32)])
        b1 = np.asarray(read_begin, dtype=np.int32); e1 = np.asarray(read_end, dtype=np.int32); rl = np.asarray(readlen, dtype=np.uint32)
        out = np.zeros((max(n, 1), 4), dtype=np.uint32)
        self._chk(self.L.smr_idcov_batch(self.h, n, rb.ctypes.data, ro.ctypes.data, fb.ctypes.data, fo.ctypes.data, cg.ctypes.data, co.ctypes.data,
                                         b1.ctypes.data, e1.ctypes.data, rl.ctypes.data, float(min_id), float(min_cov), out.ctypes.data), "smr_idcov_batch")
        return out[:n]

    def counters(self, n_db=1):
        out = (C.c_uint64 * (2 + n_db))()
        self._chk(self.L.smr_counters(self.h, out, n_db), "smr_counters")
        return dict(num_aligned=out[0], num_short=out[1], reads_matched_per_db=[out[2 + i] for i in range(n_db)])

    def counters_device(self):
        p = C.c_void_p()
        n = C.c_uint32()
        self._chk(self.L.smr_counters_device(self.h, C.byref(p), C.byref(n)), "smr_counters_device")
        return p.value, n.value

    def counters_accumulate(self, d_acc, n_u64):
        """d_acc[k] += counter k of the selected batch, k < n_u64, on the device (smr_counters_accumulate); d_acc: a device address.  k < 66:
        the block of counters_device(); k = 66 .. 69: the four sums of idcov_counters()"""
        self._chk(self.L.smr_counters_accumulate(self.h, d_acc, n_u64), "smr_counters_accumulate")

    def fetch(self):
        self._chk(self.L.smr_results_fetch(self.h), "smr_results_fetch")

    def _record(self, fn, *which):
        """the record that fn(ctx, *which, buf, cap) serialises: the call returns its size, 0 for a read without one"""
        n = fn(self.h, *which, None, 0)
        if n == 0:
            return b""
        buf = C.create_string_buffer(n)
        fn(self.h, *which, buf, n)
        return buf.raw

    def record(self, i):
        return self._record(self.L.smr_result_record, i)

    def records(self):
        return [self.record(i) for i in range(self.n_reads)]

    def record_batch(self, batch, i):
        """record of read i of batch `batch`, whichever batch is selected (smr_result_record_batch: a writer thread's call)"""
        return self._record(self.L.smr_result_record_batch, batch, i)

    def is_hit(self, i):
        return bool(self.L.smr_result_is_hit(self.h, i))

    def seed_scan(self, slot, params, strand, pass_):
        n = C.c_uint64()
        self._chk(self.L.smr_seed_scan(self.h, slot, C.byref(params), strand, pass_, C.byref(n)), "smr_seed_scan")
        return n.value

    def seed_hits(self):
        return self._fill("smr_seed_hits_fetch", lambda n, b: self.L.smr_seed_hits_fetch(self.h, *b, n), kinds=((np.uint32, 3),), always=True)

    def seed_tuples(self):
        """(sorted tuples uint64[n], cbase uint32[nc + 1], meta dict) of the last seed-stage launch (smr_seed_tuples_fetch: a test seam)"""
        meta = (C.c_uint32 * 8)()
        self._chk(self.L.smr_seed_tuples_fetch(self.h, None, 0, None, 0, meta), "smr_seed_tuples_fetch")
        tup = np.zeros(max(meta[0], 1), dtype=np.uint64)
        cbase = np.zeros(meta[2] + 1, dtype=np.uint32)
        self._chk(self.L.smr_seed_tuples_fetch(self.h, tup.ctypes.data, len(tup), cbase.ctypes.data, len(cbase), meta), "smr_seed_tuples_fetch")
        return tup[: meta[0]], cbase, dict(n=meta[0], n_fwd=meta[1], nc=meta[2], fb=meta[3], cb=meta[4], nkh=meta[5], ccap=meta[6], redo=meta[7])

    def tuning(self):
        """dict(NAME -> int) of the library's environment switches as this engine latched them when it was created (smr_tuning_text)"""
        buf = C.create_string_buffer(max(self.L.smr_tuning_text(self.h, None, 0), 1))
        self.L.smr_tuning_text(self.h, buf, len(buf))
        return {k: int(v) for k, v in (line.split("=") for line in buf.value.decode().splitlines())}

    def seed_nbmap_info(self, slot=0):
        """dict(built, drop, bytes, tries, strings, build_us, probed, passed, empty) of the search bitmap of the part in `slot` (smr_seed_nbmap_info: a
        test seam); the last three are the selected batch's counters of k_seed_pg"""
        info = (C.c_uint64 * 9)()
        self._chk(self.L.smr_seed_nbmap_info(self.h, slot, info), "smr_seed_nbmap_info")
        return dict(zip(("built", "drop", "bytes", "tries", "strings", "build_us", "probed", "passed", "empty"), (int(x) for x in info)))

    def seed_nbmap_fetch(self, slot, first, n, words_per_slab):
        """uint32[n, words_per_slab]: slabs first .. first + n - 1 of the part's search bitmap (slab 2 * key + direction)"""
        out = np.empty((n, words_per_slab), dtype=np.uint32)
        self._chk(self.L.smr_seed_nbmap_fetch(self.h, slot, first, n, out.ctypes.data_as(C.c_void_p), out.size), "smr_seed_nbmap_fetch")
        return out

    def seed_pool_info(self):
        """dict(words, grown, hi, inline) of the seed-hit pool (smr_seed_pool_info: a test seam): its size in words, its regrows since the engine
        was created, one past the highest word the last seed stage handed out, whether that stage inlined one-hit windows"""
        info = (C.c_uint64 * 4)()
        self._chk(self.L.smr_seed_pool_info(self.h, info), "smr_seed_pool_info")
        return dict(words=info[0], grown=info[1], hi=info[2], inline=bool(info[3]))

    def cand_info_enable(self, on=True):
        """switch the per-read route bytes of the candidate stage on or off for the align_part calls that follow (smr_cand_info_enable: a test seam)"""
        self._chk(self.L.smr_cand_info_enable(self.h, int(bool(on))), "smr_cand_info_enable")

    def cand_info(self):
        """dict of the last align_part's retry ladder and the context's candidate-stage capacities (smr_cand_info: a test seam): attempts,
        retries = {HITCAP, POOL, PAIRS, REDO, SCAP: attempts redone for that cause}, chain_ext, chain_scap, keys_cap, pairs_cap, hits_cap"""
        info = (C.c_uint64 * 13)()
        self._chk(self.L.smr_cand_info(self.h, info), "smr_cand_info")
        return dict(attempts=info[0], retries=dict(HITCAP=info[1], POOL=info[2], PAIRS=info[3], REDO=info[4], SCAP=info[5]), chain_ext=bool(info[6]),
                    chain_scap=info[7], keys_cap=info[8], pairs_cap=info[9], hits_cap=info[10], routes_on=bool(info[11]), routes_n=info[12])

    def cand_routes(self):
        """uint8[n_reads]: per read the ROUTE_* bits OR-ed over the launches of the last align_part's final attempt (smr_cand_routes; needs cand_info_enable)"""
        n = self.cand_info()["routes_n"]
        out = np.zeros(max(n, 1), dtype=np.uint8)
        self._chk(self.L.smr_cand_routes(self.h, out.ctypes.data, n), "smr_cand_routes")
        return out[:n]

    def prof_reset(self):
        self._chk(self.L.smr_prof_reset(self.h), "smr_prof_reset")

    def prof(self):
        p = capi.Prof()
        self._chk(self.L.smr_prof_get(self.h, C.byref(p)), "smr_prof_get")
        return p

    def prof_kernels(self):
        """{kernel family: {"ms", "launches", "bytes"}} since the last prof_reset (smr_prof_kernels)"""
        a = (capi.Kprof * 16)()
        n = C.c_uint32()
        self._chk(self.L.smr_prof_kernels(self.h, a, 16, C.byref(n)), "smr_prof_kernels")
        return {a[i].name.decode(): {"ms": a[i].ms, "launches": int(a[i].launches), "bytes": int(a[i].bytes)} for i in range(n.value)}

    def close(self):
        if self.h:
            self.L.smr_destroy(self.h)
            self.h = None


def align(engine, reads, index_parts, params_per_index, with_cigar=True, max_alignments_per_read=None, id_cov=None, resume=None, first_index_num=0):
    """processor.cpp:align(): index_parts = [[Index part0, part1, ...] per --ref], params_per_index = [Params per --ref]
    (each carrying that DB's minimal_score).  Returns nothing; results stay in `engine` (fetch()/record()).
    id_cov = (min_id, min_cov): the %id / %coverage pass (denovo_stats) over every (index, part) once all of them are aligned.
    resume = (records, counters): what records() and counters(n_db) of an earlier run over the same reads gave; imported after the upload, before
    the first part, so that this call continues that run on further --ref (counters: the dict of counters(n_db), or None to leave them at 0).
    first_index_num: the index_num of index_parts[0] -- the number of --ref the earlier run went through."""
    if id_cov is not None and not with_cigar:
        raise SmrError("align: id_cov needs the CIGARs (with_cigar=True)")
    if id_cov is not None and resume is not None:
        raise SmrError("align: id_cov with resume is not supported here (the pass needs the references of the earlier --ref as well)")
    p0 = params_per_index[0]
    slots = max_alignments_per_read or (p0.num_alignments if p0.num_alignments > 0 else 32)
    if reads is not None:                       # (None: the selected batch is in place already, e.g. by engine.upload_fastx with as many slots)
        engine.upload_reads(reads, slots)
    if resume is not None:
        records, counters = resume
        engine.import_state(records)
        if counters is not None:
            engine.import_counters(counters, len(counters["reads_matched_per_db"]) if isinstance(counters, dict) else len(counters) - 2)
    n_idx = len(index_parts)
    single = sum(len(parts) for parts in index_parts) == 1
    for idx_num, parts in enumerate(index_parts):
        for part, ix in enumerate(parts):
            p = params_per_index[idx_num]
            p.index_num = first_index_num + idx_num
            p.part = part
            p.is_last_index_part = int(idx_num == n_idx - 1 and part == len(parts) - 1)
            engine.upload_index(ix, 0)
            engine.align_part(0, p)
            if with_cigar:
                engine.traceback(0, p)
            if id_cov is not None and single:
                engine.idcov_part(0, p, id_cov[0], id_cov[1])
            engine.unload_index(0)
    if id_cov is not None and not single:
        # the pass counts the FINAL alignments (the reference's denovo_stats runs after align): every part's references once more
        for idx_num, parts in enumerate(index_parts):
            for part, ix in enumerate(parts):
                p = params_per_index[idx_num]
                p.index_num = first_index_num + idx_num
                p.part = part
                engine.upload_index(ix, 0)
                engine.idcov_part(0, p, id_cov[0], id_cov[1])
                engine.unload_index(0)
    engine.fetch()


def align_resident(engine, index_slots, params_per_index, with_cigar=True, id_cov=None):
    """Same loop over (index, part) for reads AND index parts that are already resident in HBM: index_slots is either a
    flat list of slots (one --ref, its parts in order) or a list of such lists (one per --ref).  Acts on the selected
    batch; the caller resets its state first when the batch is reused."""
    if index_slots and not isinstance(index_slots[0], (list, tuple)):
        index_slots = [index_slots]
    n_idx = len(index_slots)
    for idx_num, slots in enumerate(index_slots):
        for part, slot in enumerate(slots):
            p = params_per_index[idx_num]
            p.index_num = idx_num
            p.part = part
            p.is_last_index_part = int(idx_num == n_idx - 1 and part == len(slots) - 1)
            engine.align_part(slot, p)
            if with_cigar:
                engine.traceback(slot, p)
    if id_cov is not None:
        if not with_cigar:
            raise SmrError("align_resident: id_cov needs the CIGARs (with_cigar=True)")
        for idx_num, slots in enumerate(index_slots):
            for part, slot in enumerate(slots):
                p = params_per_index[idx_num]
                p.index_num = idx_num
                p.part = part
                engine.idcov_part(slot, p, id_cov[0], id_cov[1])
    engine.fetch()
