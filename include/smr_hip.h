/*
 * smr_hip.h -- C ABI of libsmr_hip.so: the MI355X (gfx950) engine for SortMeRNA's per-read hot path.
 *
 * This is the drop-in boundary.  The reference is one C++17 executable with no plugin
 * API; the seam is the per-read call  traverse(opts, index, refs, readstats, refstats, read, isLastStrand)
 * made from align2()  (/root/reference/src/sortmerna/processor.cpp:85,104-161), once per
 * read x strand x index part, by the thread pool of align() (processor.cpp:173-285).  A maintainer
 * replaces that loop by batch calls into this library (binding sketch: INTEGRATION.md).
 *
 * Everything here is plain C: pointers, sizes, int error codes (0 = ok, <0 = error, message via
 * smr_last_error).  No exceptions, no C++ or torch types cross the ABI.
 *
 * What each entry point replaces in the reference:
 *   smr_index_*      Index::load + References::load          index.cpp:143-357, references.cpp:55-159
 *                    (+ our own builder = build_index()       indexdb.cpp:1119-2095)
 *   smr_reads_*      Readfeed::next -> Read(readstr).init()   readfeed.hpp:124, read.cpp:264-347
 *   smr_refstats_*   Refstats::load (.stats + minimal_score)  refstats.cpp:103-265  (Gumbel lambda,K are INPUTS:
 *                    the reference gets them from the vendored NCBI ALP library, refstats.cpp:194-233)
 *   smr_align_part   the N x align2() threads for one (index, part): traverse() -> traversetrie_align()
 *                    -> compute_lis_alignment() -> ssw_align()   paralleltraversal.cpp:81-298,
 *                    traverse_bursttrie.cpp:100-298, alignment.cpp:100-509, ssw.c:834-941
 *   smr_result_*     Read::toBinString() / kvdb.put()         read.cpp:429-462, processor.cpp:150-155
 *   smr_counters     Readstats atomics                        readstats.hpp:77-85
 *   smr_state_import  Read::load_db  read.cpp:467-539, processor.cpp:116-126
 *   smr_state_export  Read::toBinString  read.cpp:429-462, for a whole batch
 *   smr_idcov_*      denovo_stats: %id / %coverage of every stored alignment, the four per-read and Readstats counters of -otu_map / -de_novo_otu
 *                    processor.cpp:287-438, Read::calc_miss_gap_match read.cpp:547-589
 *
 * Hard limits of this build (each is an explicit error -- SMR_ERR_CAPACITY / SMR_ERR_ARG with a message --, never a silent difference):
 *   reads                 <= 65 535 letters each; reads x windows of the finest pass < 2^31 per batch (150-nt reads: ~47 M; the benches use 8 M)
 *   resident batches      16 per context (smr_batch_select), resident index parts 64 per context (smr_index_upload slot 0..63)
 *   seed length           8..20, even; < 2^31 - 1 distinct seeds (ids) per index part
 *   seed hits             no limit: the lane-local hit lists grow to what a half-seed search can accept at most (31 L/2 - 20 strings, smr_prof.hit_list_cap)
 *   candidate references  <= 49 152 references that occur at least twice among the seed positions of ONE read on one strand (3/4 of the 65 536 slots of
 *                         the per-block global table of k_chain<EXT>; the 49 153rd is SMR_ERR_CAPACITY, the context stays usable: tests/test_gpu_cand_limits.py);
 *                         (a lower bound of what counts: a reference that occurs once is a member too when its bit of the set's Bloom filter collides,
 *                         which is why the error message speaks of references that "share seeds with one read");
 *                         up to 384 of them stay in the LDS table of a wave, the first read with more switches the context to the global tables (one retry)
 *   alignments per read   max_alignments_per_read given to smr_reads_upload (the reference's -num_alignments, or 256 for "all")
 *   scoring               match <= 127, |mismatch|, |score_N| <= 127, gaps <= 255.  With 2 * gap_open, 2 * gap_ext >= |mismatch|, gap_open > gap_ext and score_N <= 0 the
 *                         affine recurrence of the fast kernels equals the reference's striped kernels cell for cell; outside those conditions ssw.c's scores
 *                         depend on its SIMD stripe geometry (ssw.c:267,496 and its 16-bit lazy-F loop :496-507), and smr_align_part scores through a slow
 *                         path that reproduces that geometry (csrc/smr_sw_striped.hpp; about ten times slower; rounds 1 - 5 refused such schemes)
 *   edges                 1..10 letters or percent like the reference's --edges; a percentage must not round to 0 letters for any searchable read of the batch
 *   pools                 seed-hit pool <= 8 GiB, CIGAR pool < 2^32 words, pigeonhole arena < 2^34 words per part (all grown on demand)
 */
#ifndef SMR_HIP_H
#define SMR_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMR_OK 0
#define SMR_ERR_ARG (-1)        /* bad argument / unsupported option value */
#define SMR_ERR_IO (-2)         /* file missing or malformed */
#define SMR_ERR_DEVICE (-3)     /* HIP error (no GPU, out of memory, kernel fault) */
#define SMR_ERR_CAPACITY (-4)   /* a device pool overflowed after automatic regrow attempts */
#define SMR_ERR_STATE (-5)      /* call order violated */

typedef struct smr_ctx smr_ctx;          /* one GPU: stream, resident index parts, resident read batch */
typedef struct smr_index smr_index;      /* HOST: one flattened index part + its reference sequences */
typedef struct smr_reads smr_reads;      /* HOST: a packed read batch */

/* Options of Runopts that reach the hot path (include/options.hpp:495-608; defaults options.cpp:1566-1758). */
typedef struct {
  uint32_t skiplengths[3];   /* -passes      pass strides; {0,0,0} => {L, L/2, 3}     refstats.cpp:159-166 */
  int32_t  num_seeds;        /* -num_seeds   2 */
  int32_t  min_lis;          /* -min_lis     2 */
  int32_t  edges;            /* -edges       4 */
  int32_t  is_as_percent;    /* -edges N%    0 */
  int32_t  match;            /* -match       2 */
  int32_t  mismatch;         /* -mismatch   -3 */
  int32_t  score_N;          /* -N           = mismatch */
  int32_t  gap_open;         /* -gap_open    5 */
  int32_t  gap_ext;          /* -gap_ext     2 */
  uint32_t num_alignments;   /* -num_alignments 1 (0 = all) */
  int32_t  is_best;          /* 1 unless -no-best */
  int32_t  is_full_search;   /* -full_search 0 */
  int32_t  is_forward;       /* -F */
  int32_t  is_reverse;       /* -R  (both 1 when neither given) */
  uint32_t minoccur;         /* 0 */
  /* per call of smr_align_part: */
  uint32_t minimal_score;    /* Refstats::minimal_score[index_num]            refstats.cpp:261-265 */
  uint32_t index_num;        /* position of the DB in --ref order */
  uint32_t part;             /* index part number */
  int32_t  is_last_index_part; /* last part of the last index                 paralleltraversal.cpp:294 */
} smr_params;

void smr_params_default(smr_params* p);
/* NULL when smr_align_part takes these options; otherwise the reason it will answer SMR_ERR_ARG (--edges outside 1..10: INTEGRATION.md "known
 * limits").  For a host's option parser, so that a driver says so before it loads anything.  (Scoring schemes under which ssw.c's striped kernels
 * leave the affine recurrence are no longer among them: round 6 scores them through the slow path of csrc/smr_sw_striped.hpp.) */
const char* smr_params_refused(const smr_params* p);

/* ------------------------------------------------------------------------------------------------
 * Index (host side).  An smr_index is one (index, part): 9-mer lookup, mini burst tries in a compact
 * word arena, positions CSR, reference sequences (0..4, 1 byte/nt).
 * ---------------------------------------------------------------------------------------------- */
/* Load a part written by the reference's indexer: <prefix>.kmer_P.dat / .bursttrie_P.dat / .pos_P.dat
 * (+ <prefix>.stats for the part's byte range in the FASTA).  Replaces Index::load + References::load. */
int smr_index_load_files(const char* prefix, uint32_t part, const char* ref_fasta, smr_index** out, char* err, size_t errcap);

/* Build ALL parts of the index of one FASTA ourselves (replaces build_index(), indexdb.cpp:1119-2095):
 * same 19-mer geometry, same forward/reverse mini-trie contents, ids = rank of the unique 18-mer
 * (any bijection is equivalent: ids are opaque keys into the positions table), positions in file
 * order truncated at max_pos.  n_parts_out parts are returned in parts_out[0..n_parts_out).
 * max_file_size_mb = the reference's -m (3072), seed_win_len = -L (18), max_pos = -max_pos (10000). */
int smr_index_build(const char* ref_fasta, uint32_t seed_win_len, double max_file_size_mb, uint32_t max_pos,
                    uint32_t threads, smr_index** parts_out, uint32_t cap_parts, uint32_t* n_parts_out,
                    char* err, size_t errcap);
/* Write one part in the REFERENCE's on-disk format (so the reference binary can consume our index). */
int smr_index_write_files(const smr_index* const* parts, uint32_t n_parts, const char* ref_fasta, const char* prefix,
                          char* err, size_t errcap);
/* Flat cache of one part's HOST layout (header + the arrays as they lie in memory, page aligned): smr_index_load_flat maps the file and
 * copies the arrays with all cores -- the reference-format files store no stream lengths (index.cpp:176-316) and cost a sequential walk
 * over GBs plus a parse (1.3 s for the 140 Mnt DB, 0.3 s from the cache).  `stamp` is the caller's key for "these reference files" (size
 * and mtime, a hash ...): load returns SMR_ERR_STATE when the file was written under another stamp, SMR_ERR_IO when it is absent or damaged;
 * the caller then loads the reference's files (or builds) and saves the cache for the next run. */
int smr_index_save(const smr_index*, const char* path, uint64_t stamp, char* err, size_t errcap);
int smr_index_load_flat(const char* path, uint64_t stamp, smr_index** out, char* err, size_t errcap);
/* Consistency check of the two device layouts of the mini-tries (reference-shaped arena for k_seed_search, pigeonhole arena for
 * k_seed_pg): the second must hold the same (candidate string, id) entries with their ranks in the DFS order of the first, sorted by its
 * two keys, under consistent directories.  0 = ok. */
int smr_index_selfcheck(smr_index*, char* err, size_t errcap);
void smr_index_free(smr_index*);

typedef struct {
  uint32_t lnwin;            /* L */
  uint32_t n_kmers;          /* 4^(L/2) */
  uint64_t trie_words;       /* u32 words in the mini-trie arena */
  uint32_t n_ids;            /* unique 18-mers */
  uint64_t n_pos;            /* total positions */
  uint32_t n_refs;           /* sequences in this part */
  uint64_t ref_bytes;        /* total nt in this part */
  uint64_t n_nodes, n_buckets, n_entries;
  double   bg[4];            /* A,C,G,T background frequencies of the whole DB (from .stats / builder) */
  uint64_t full_len;         /* total nt of the whole DB */
  uint64_t numseq;           /* total sequences of the whole DB */
  uint32_t n_parts;
} smr_index_info;
int smr_index_get_info(const smr_index*, smr_index_info* out);

/* Refstats::load arithmetic (refstats.cpp:238-265): minimal SW score for E-value `evalue` given the
 * Gumbel parameters of the (scoring scheme, background) pair and the GLOBAL read totals
 * (all_reads_count / all_reads_len are sums over every rank when reads are sharded).
 * lambda and K are INPUTS and there is no default: the reference computes them per DB and scoring scheme (-match / -mismatch / -gap_open /
 * -gap_ext, background frequencies) with its vendored NCBI ALP library (refstats.cpp:194-233) and prints them in its log ("Gumbel lambda",
 * "Gumbel K").  A different pair gives a different minimal_score, i.e. a different set of reads passes -- take them from the reference
 * (the compiled drop-in of INTEGRATION.md uses the reference's own Refstats object). */
uint32_t smr_minimal_score(double lambda, double K, const double bg[4], uint64_t full_ref_len, uint64_t numseq,
                           uint64_t all_reads_count, uint64_t all_reads_len, double evalue);
/* The same under -score_split (refstats.cpp:247: `full_read_scale = opts.is_score_split ? opts.num_proc_thread : 1`): the read totals are
 * divided by the number of processing threads the reference was run with; full_read_scale = 1 is smr_minimal_score. */
uint32_t smr_minimal_score_split(double lambda, double K, const double bg[4], uint64_t full_ref_len, uint64_t numseq,
                                 uint64_t all_reads_count, uint64_t all_reads_len, double evalue, uint32_t full_read_scale);

/* The length-corrected database / read sizes of Refstats (refstats.cpp:238-257) that the e-value of the BLAST report uses. */
void smr_refstats_corrected(double K, const double bg[4], uint64_t full_ref_len, uint64_t numseq, uint64_t all_reads_count, uint64_t all_reads_len,
                            uint64_t* full_ref_corr, uint64_t* full_read_corr);
void smr_refstats_corrected_split(double K, const double bg[4], uint64_t full_ref_len, uint64_t numseq, uint64_t all_reads_count, uint64_t all_reads_len,
                                  uint32_t full_read_scale, uint64_t* full_ref_corr, uint64_t* full_read_corr);

/* ------------------------------------------------------------------------------------------------
 * Reads (host side): 2-bit packed + ambiguity mask (Read::seqToIntStr: ACGT(U) -> 0..3, other -> 0
 * and the position is remembered, read.cpp:334-347).
 * ---------------------------------------------------------------------------------------------- */
/* seqs: concatenated ASCII sequences, offs[n+1] byte offsets. */
int smr_reads_pack(const char* seqs, const uint64_t* offs, uint32_t n_reads, smr_reads** out);
/* FASTA/FASTQ (optionally multi-line FASTA), plain text; [first, first+count) selects a record range
 * (count = 0 => to the end): the host-side read shard of one rank. */
int smr_reads_load_fastx(const char* path, uint64_t first, uint64_t count, smr_reads** out, char* err, size_t errcap);
/* The whole file (plain or gzip, izlib.cpp:95-210), parsed and packed by `threads` threads (0 = all cores) over byte ranges that start at record boundaries (the
 * reference splits the read file the same way into one range per thread, readfeed.cpp:1253-1277).  Same result as
 * smr_reads_load_fastx(path, 0, 0, ...). */
int smr_reads_load_fastx_mt(const char* path, uint32_t threads, smr_reads** out, char* err, size_t errcap);
void smr_reads_free(smr_reads*);
/* records [first, first + count) of a packed batch as a batch of their own (no text): the host-side split of the reads into one shard per
 * GPU (the reference splits the read file into one range per thread, readfeed.cpp:1253-1277) or into the chunks of an upload/align pipeline */
int smr_reads_slice(const smr_reads*, uint64_t first, uint64_t count, smr_reads** out);
/* like smr_reads_load_fastx_mt, and keeps the file text so that smr_reads_record_text can hand out every record's header line (as in the
 * file, with '>' / '@'), letters (line breaks removed) and quality line for the report writers; lens = {header, letters, quality} lengths;
 * a NULL / too small buffer is skipped / filled as far as it goes (always NUL-terminated) */
int smr_reads_load_fastx_text(const char* path, uint32_t threads, smr_reads** out, char* err, size_t errcap);
int smr_reads_is_fastq(const smr_reads*);
int smr_reads_record_text(const smr_reads*, uint32_t i, char* hdr, size_t hdr_cap, char* seq, size_t seq_cap, char* qual, size_t qual_cap, size_t lens[3]);
uint64_t smr_reads_digest(const smr_reads*);   /* hash of the packed batch (lengths, offsets, words): equal digests = same reads, same order */
uint32_t smr_reads_count(const smr_reads*);
uint64_t smr_reads_total_len(const smr_reads*);
uint32_t smr_reads_min_len(const smr_reads*);
uint32_t smr_reads_max_len(const smr_reads*);

/* ------------------------------------------------------------------------------------------------
 * Device context
 * ---------------------------------------------------------------------------------------------- */
int  smr_device_count(void);   /* HIP devices this process sees (0: none -- there is no CPU fallback); a host that spreads its read chunks over the GPUs of a node creates one context per device (the reference: one aligner thread per core, processor.cpp:248-256) */
int  smr_create(int device, smr_ctx** out, char* err, size_t errcap);
void smr_destroy(smr_ctx*);
const char* smr_last_error(const smr_ctx*);
/* The environment switches of the library as this context latched them in smr_create (every switch of a context is read there, once; clamped):
 * one NAME=value line per switch, NUL-terminated.  Returns the size needed (the buffer is filled when it is large enough) or SMR_ERR_ARG.
 * INTEGRATION.md lists the names, defaults and meanings. */
int  smr_tuning_text(const smr_ctx*, char* buf, size_t cap);

/* Copy an index part to HBM; it stays resident under `slot` (0..63) until freed. */
int smr_index_upload(smr_ctx*, const smr_index*, int slot);
/* Test seam: the pigeonhole layout that smr_index_upload BUILT ON THE DEVICE for `slot` (from the uploaded lookup table and mini-trie arena;
 * it replaces a host pass over every mini-trie, indexdb.cpp's in-memory tries being what both start from) against the host transform of the
 * same index, word for word.  SMR_PG_HOST=1 makes smr_index_upload use the host transform instead. */
int smr_index_check_device(smr_ctx*, int slot, smr_index*);
/* Test seams of the roofline numerator's audit (tests/test_gpu_parity.py::test_pigeonhole_search_bytes_equal_a_host_recount): the pigeonhole
 * layout of a host index as the host transform builds it, and the sorted tuples of the context's last seed-stage launch with what decodes them
 * (meta = {tuples, forward tuples, coarse bins, fine key bits, char bits, forward keys, candidate records per wave, waves handed to the DFS kernel}). */
int smr_index_pigeonhole(smr_index*, const uint32_t** pg, uint64_t* pg_words, const uint32_t** root3, uint64_t* root3_words, char* err, size_t errcap);
int smr_seed_tuples_fetch(smr_ctx*, uint64_t* tuples, uint64_t cap_tuples, uint32_t* cbase, uint32_t cap_cbase, uint32_t meta[8]);
/* Test seam of the seed-hit pool (SMR_SEED_POOL_WORDS=<n> starts it at n words, clamped to [64, 0x7FFFFFF0]): info = {pool words, regrows
 * since smr_create, one past the highest pool word the selected batch's last seed stage handed out, 1 if that stage inlined one-hit windows}. */
int smr_seed_pool_info(smr_ctx*, uint64_t info[4]);
/* Test seams of the search bitmap (SMR_SEED_NBMAP, csrc/smr_nbmap.hpp).  smr_seed_nbmap_info: info = {1 if the part in `slot` has a bitmap, pattern
 * chars it leaves out, its bytes, present mini-tries of the part, their strings, microseconds of the builder kernel, then from the selected batch's
 * counters: searches probed, searches whose bit was set, searches of those that accepted no string}; an empty slot gives zeros for the part.
 * The three count the chunks k_seed_pg finished itself: a wave chunk handed to the DFS kernel (candidate pool overflow) or made of repeated seeds only is in none of them.
 * smr_seed_nbmap_fetch: slabs [first, first + n)
 * of the part's bitmap (slab 2 * key + direction, 4^(partialwin - chars left out) / 32 words each). */
int smr_seed_nbmap_info(smr_ctx*, int slot, uint64_t info[9]);
int smr_seed_nbmap_fetch(smr_ctx*, int slot, uint64_t first, uint64_t n, uint32_t* out, uint64_t cap_words);
/* Test seam of the candidate stage (tests/test_gpu_cand_limits.py).  smr_cand_info: info = {attempts of the last smr_align_part, how many of them
 * were redone because of HITCAP, POOL, PAIRS, REDO, SCAP (five words), then chain_ext, chain_scap, keys_cap, pairs_cap, hits_cap of the context as
 * they stand, 1 if the route bytes are switched on, the number of reads they cover}.  After smr_cand_info_enable(ctx, 1) every smr_align_part also
 * keeps one byte per read, OR-ed over the (strand, pass) launches of its final attempt, which smr_cand_routes copies out (n = reads of the batch):
 * SMR_ROUTE_RECORD / SMR_ROUTE_GATHER = listed for the walk rounds with / without a record of k_cand, SMR_ROUTE_CHAIN = walked by k_chain on its
 * wave's LDS table, SMR_ROUTE_EXT = by its second launch on the block's global table.  Switched off (the default) no kernel is launched for it. */
#define SMR_ROUTE_RECORD 1u
#define SMR_ROUTE_GATHER 2u
#define SMR_ROUTE_CHAIN 4u
#define SMR_ROUTE_EXT 8u
int smr_cand_info_enable(smr_ctx*, int on);
int smr_cand_info(smr_ctx*, uint64_t info[13]);
int smr_cand_routes(smr_ctx*, uint8_t* out, uint32_t n);
int smr_index_unload(smr_ctx*, int slot);

/* Several read batches (0..15) can be resident at once, so the host can upload batch k+1 while batch k is being
 * aligned (the reference's Readfeed hands reads to align2() one at a time, processor.cpp:104; here the unit is a
 * batch).  smr_batch_select picks the batch every later call acts on (default 0).  Each batch owns its per-read
 * state, its Readstats counter block and its CIGAR pool; the caller sums the counters of its batches. */
int smr_batch_select(smr_ctx*, int batch);

/* Seed-search kernel selection.  0 (default): the pigeonhole kernel k_seed_pg.  1: the per-lane DFS kernel k_seed_search for
 * every window; slower, but its work counters (smr_prof_get: n_node, n_entry) follow the reference's sequential scan exactly
 * (nothing after a 0-error match is counted) -- used to obtain the algorithmic byte counts of a workload.  Results are identical. */
int smr_set_seed_mode(smr_ctx*, int exact_counters);

/* Copy a read batch to HBM (into the selected batch) and allocate its persistent per-read state (what the reference keeps in
 * the KVDB between index parts, read.cpp:429-539).  Resets all state and counters. */
int smr_reads_upload(smr_ctx*, const smr_reads*, uint32_t max_alignments_per_read);
/* The same into batch `batch` (0..15) WITHOUT selecting it, on the context's second (upload) stream: a second host thread may call this
 * while the first one is inside smr_align_part / smr_traceback / smr_results_fetch of another batch -- upload of batch k+1 overlaps the
 * alignment of batch k (the reference's Readfeed/Processor overlap file reading with alignment the same way, readfeed.cpp, processor.cpp:248-256).
 * Fails with SMR_ERR_STATE when `batch` is the selected batch. */
int smr_reads_upload_batch(smr_ctx*, int batch, const smr_reads*, uint32_t max_alignments_per_read);
/* FASTA/FASTQ TEXT to a resident batch: records are found, measured, laid out and 2-bit packed by kernels (csrc/smr_fastx.hpp), straight into the
 * batch's device arrays.  For any bytes the batch -- and *out -- are exactly what smr_reads_load_fastx_text + smr_reads_upload of a file holding
 * those bytes give, including the error code and message of malformed text (smr_last_error; no file name in front for the two buffer calls).
 * Regular text is handled on the device: any FASTA, and FASTQ in which, counting lines from the first byte that is not '\n' / '\r', every line 4k
 * begins with '@' up to the last record, the record count is whole and only lines that are empty or one '\r' follow.  Anything else (blank lines
 * between FASTQ records, a cut last record, stray bytes, empty text) is walked by the host parser inside the same call ("Parsing
 * and packing on the device").  n_bytes >= 2^32 - 64 is SMR_ERR_CAPACITY, decided before the text is touched: hand the text over in pieces that
 * end at record boundaries.  After a refusal the batch is as it was before the call.
 *   smr_reads_upload_fastx        into the selected batch, on the engine's stream
 *   smr_reads_upload_fastx_batch  into batch `batch` on the upload stream, like smr_reads_upload_batch (SMR_ERR_STATE for the selected batch)
 *   smr_reads_upload_fastx_file   maps the file (inflates a gzip file) first; the message also goes to err
 * out == NULL: only the totals come back from the device.  Otherwise *out is a complete smr_reads (smr_reads_free it): lengths, offsets and packed
 * words are copied back from the device, so smr_reads_digest, _slice, _record_text, ... work on it unchanged.  With the two buffer calls its
 * text borrows the caller's bytes, which must outlive it; the file call's object owns the text.
 * flags & SMR_FASTX_VIEW: the packed words are not copied back.  The object has the text, the record offsets, lengths and statistics:
 * smr_reads_record_text, _count, _total_len, _min_len, _max_len and _is_fastq work; smr_reads_slice and smr_reads_upload* answer SMR_ERR_STATE and
 * smr_reads_digest answers 0.
 * flags & SMR_FASTX_KEEP (combines with SMR_FASTX_VIEW): the text stays with the batch on the device -- the padded text, the offsets of every
 * record's header line and first sequence line, the format: what smr_reads_record_text reads -- for smr_fastx_split.  The buffers the parser
 * kernels worked on are handed over, not copied (the upload's scratch allocates again on its next use); text the host parser walked is
 * uploaded with the parser's offsets.  Cost: the text plus 16 bytes per record of device memory until the batch is uploaded into again by any
 * upload call (which drops it) or the context is destroyed; smr_state_reset keeps it.  Without the flag nothing is kept and nothing changes.
 * flags & SMR_FASTX_INFLATE (combines with both): bytes that begin 1f 8b are a gzip file; they go to the device compressed (the file call's
 * straight from the mapping), are inflated there into the text buffer (smr_gunzip_batch below says how, and when the host inflates instead)
 * and parsed from it: the H2D of the text disappears.  With out != NULL the inflated text is copied back once, into a buffer *out owns (also
 * under the two buffer calls); with out == NULL only the totals cross the bus.  Inflated text of 2^32 - 64 bytes or more is SMR_ERR_CAPACITY.
 * A file zlib refuses is SMR_ERR_IO with zlib's verdict ("<path>: truncated gzip stream", "<path>: corrupt gzip stream"), as without the
 * flag.  Without the flag, or for bytes that are not gzip, nothing changes. */
#define SMR_FASTX_VIEW 1u
#define SMR_FASTX_KEEP 2u
#define SMR_FASTX_INFLATE 4u
int smr_reads_upload_fastx(smr_ctx*, const char* text, uint64_t n_bytes, uint32_t max_alignments_per_read, uint32_t flags, smr_reads** out);
int smr_reads_upload_fastx_batch(smr_ctx*, int batch, const char* text, uint64_t n_bytes, uint32_t max_alignments_per_read, uint32_t flags, smr_reads** out);
int smr_reads_upload_fastx_file(smr_ctx*, const char* path, uint32_t max_alignments_per_read, uint32_t flags, smr_reads** out, char* err, size_t errcap);
/* Test seam (tests/test_gpu_fastx_device.py): of the last smr_reads_upload_fastx* call on the context {path taken: 0 the kernels, 1 the host parser;
 * lines the kernels found; records; text bytes copied to the device}.  smr_fastx_times: HIP-event milliseconds of that call's stages on the
 * device path {text H2D, lines, records, pack, results D2H} (0 for the host parser's path). */
int smr_fastx_info(const smr_ctx*, uint64_t info[4]);
int smr_fastx_times(const smr_ctx*, double ms[5]);
/* The aligned.* / other.* FASTX outputs of the selected batch, written on the device (csrc/smr_fxsplit.hpp) from the text that SMR_FASTX_KEEP
 * left there and the batch's per-read is_hit: what smr_results_fetch + smr_reads_record_text + smr_report_add / smr_report_add_pair write one
 * read at a time ("Writing aligned.* / other.* from the device").  Eight streams, aligned[0..3] then other[0..3]; index j is the
 * file smr_report_open gives that index (the only file; _fwd / _rev; _paired / _singleton; _paired_fwd, _paired_rev, _singleton_fwd,
 * _singleton_rev).  Stream k is bytes[off[k], off[k + 1]), off[0] = 0, off[8] = *need; a stream that does not exist under the options, or is
 * not wanted, is empty.  Each stream holds exactly the bytes the host writer puts into that file when it is given the reads in order: per record
 * the header line, the letters of all sequence lines joined, and for FASTQ "+" and the quality line, each trimmed of trailing '\r', blank and tab
 * and ended by '\n'.  Routing: layout 0 smr_report_add, layouts 1 and 2 the table of smr_report_add_pair.
 *   hit    NULL: the batches' own is_hit (before any alignment every read is `other`).  Else one byte per read, non-zero = aligned: the reads of
 *          the selected batch, then -- layout 2 -- those of batch `mates`; used instead of the device's.
 *   bytes  NULL: sizes only.  cap < *need: SMR_ERR_CAPACITY, off and *need valid, bytes untouched.  Otherwise exactly *need bytes are written.
 *          May be pinned memory.
 * SMR_ERR_STATE (the message names SMR_FASTX_KEEP) for a batch without kept text.  SMR_ERR_ARG under layouts 1 and 2 for an odd read count
 * (layout 1), `mates` equal to the selected batch, unequal read counts or FASTA against FASTQ (layout 2), and the option combinations
 * smr_report_open refuses.  Runs on the engine's stream; needs no smr_results_fetch and leaves the host copy of the results alone; may be
 * repeated.  Device memory: 24 bytes per record of scratch and the output, both kept for the next call. */
typedef struct {
  int32_t layout;      /* 0: single reads; 1: mates interleaved in the selected batch (2i, 2i+1); 2: mates of read i of the selected batch are read i of batch `mates` */
  int32_t paired_in, paired_out, out2, sout;   /* as in smr_report_opts */
  int32_t want_aligned, want_other;            /* -fastx / -other: a stream that is not wanted has length 0 */
} smr_fxsplit_opts;
int smr_fastx_split(smr_ctx*, int mates /* batch number, layout 2 only; else -1 */, const smr_fxsplit_opts*,
                    const uint8_t* hit /* NULL: the batches' own is_hit */, uint8_t* bytes, uint64_t cap, uint64_t off[9], uint64_t* need);
/* HIP-event milliseconds of the last smr_fastx_split: {measure and route, scans, copy, bytes D2H} (the last two 0 for a sizes-only call) */
int smr_fastx_split_times(const smr_ctx*, double ms[4]);
/* The rows of aligned.sam and of the BLAST tabular report (-blast '1 ...') of the selected batch for ONE (index, part), written on the device
 * (csrc/smr_rows.hpp) from the text that SMR_FASTX_KEEP left there, the packed letters, the stored alignments with their CIGARs and the part's
 * reference letters: what smr_results_fetch + smr_reads_record_text + smr_result_record + smr_report_add append to the report's rows of that
 * (index, part) one read at a time ("Writing SAM and BLAST rows from the device").  Call order as smr_idcov_part: after
 * smr_align_part + smr_traceback of every (index, part) of the run, once per (index, part) with that part resident in `slot`; `ix` is the host
 * object of that part (its sq_header gives the reference ids; they are uploaded the first time the call sees the slot and go with the slot).
 * Two streams: the SAM rows are bytes[off[0], off[1]), the BLAST rows bytes[off[1], off[2]), off[0] = 0, off[2] = *need; a stream that is not
 * wanted is empty.  Each holds exactly the bytes the host writer appends for the reads of the batch in order: rows in read order, within a read
 * in alignment-slot order, alignments of other (index, part) keys skipped; no SAM header lines.  That includes the writer's quirk with QUAL (one
 * copy of the quality per key, reversed in place at every reverse-strand alignment of the key) and `%.3g` of %id and qcov, whose digits are
 * found in exact integer arithmetic on the double.  BLAST pairwise (-blast 0) has its own call, smr_pairwise_part below.
 *   bytes  NULL: sizes only.  cap < *need: SMR_ERR_CAPACITY, off and *need valid, bytes untouched.  Otherwise exactly *need bytes are written
 *          and nothing behind them is touched.  May be pinned memory.
 * SMR_ERR_STATE: a batch without kept text (the message names SMR_FASTX_KEEP); an alignment of the part without a CIGAR (smr_traceback first).
 * SMR_ERR_ARG: neither stream wanted; an unknown word in blast_cols; `ix` is not the part in `slot`; and -- checked on the device before any
 * byte is written, imported state can hold them and the host writer would read out of bounds -- a CIGAR without columns, a CIGAR that runs
 * past its read or its reference sequence, ref_num >= the part's references.  Every refusal leaves a message, writes nothing and leaves the
 * context usable.  Runs on the engine's stream; needs no smr_results_fetch and leaves the host copy alone; changes no stored state (it does not
 * mark alignments as smr_idcov_part does); may be repeated and gives the same bytes.  Device memory, kept for the next call: 16 bytes per
 * alignment slot, 32 per read, the output. */
typedef struct {
  int  want_sam, want_blast;       /* BLAST tabular only */
  char blast_cols[64];             /* as smr_report_opts.blast_cols: "cigar", "qcov", "qstrand", space separated, in output order */
  double lambda, K;                /* as smr_report_set_db: e-value and bit score of the BLAST row */
  uint64_t full_ref_corr, full_read_corr;
} smr_rows_opts;
int smr_rows_part(smr_ctx*, int slot, const smr_params*, const smr_index* ix, const smr_rows_opts*,
                  uint8_t* bytes, uint64_t cap, uint64_t off[3], uint64_t* need);
/* HIP-event milliseconds of the last smr_rows_part: {alignment statistics, sizes and scans, write, bytes D2H} (the last two 0 for a sizes-only call) */
int smr_rows_times(const smr_ctx*, double ms[4]);
/* Test seam of the device's number formatter: out[16 i ..] = the text of `stream << (double)num[i] / (double)den[i] * 100` at precision 3
 * (`%.3g`), NUL padded, for n pairs with den > 0 (SMR_ERR_ARG otherwise). */
int smr_rows_fmt_batch(smr_ctx*, uint32_t n, const uint32_t* num, const uint32_t* den, char* out);
/* The BLAST-like pairwise text (-blast 0) of the selected batch for ONE (index, part), written on the device (csrc/smr_pairwise.hpp) from what
 * smr_rows_part reads ("Writing the BLAST pairwise report from the device").  Call order and the meaning of slot / params / ix
 * as smr_rows_part: the key is index_num and part of the params; lambda, K and the two corrected sizes as given to smr_report_set_db.  The
 * stream holds exactly what the host writer (smr_report_add of a report opened with blast_pairwise) appends for the reads of the batch in order:
 * blocks in read order, within a read in alignment-slot order, alignments of other (index, part) keys skipped.  A block: "Sequence ID: <ref
 * id>", "Query ID: <read id>", the score line (score1, bit score, e-value, strand; both texts from the table smr_rows_part builds, the device
 * formats no float), then for every 60 alignment columns the Target line, the marks and the Query line, each letter line between its first
 * 1-based position (setw 8 / 9, never truncated) and the running 0-based position behind the chunk -- which for a chunk made of insertions
 * only is one less than the Target line's first number, as the host prints it.
 *   bytes  NULL: the size only.  cap < *need: SMR_ERR_CAPACITY, *need valid, bytes untouched.  Otherwise exactly *need bytes are written and
 *          nothing behind them is touched.  May be pinned memory.  Offsets are 64 bit.
 * SMR_ERR_STATE: a batch without kept text (the message names SMR_FASTX_KEEP); an alignment of the part without a CIGAR (smr_traceback first).
 * SMR_ERR_ARG: `ix` is not the part in `slot`; an e-value or bit-score text too long for the table; and -- counted on the device before any
 * byte is written -- a CIGAR without columns, a CIGAR that runs past its read or its reference sequence, ref_num >= the part's references.
 * Every refusal leaves a message that names the call, writes nothing and leaves the context usable.  Runs on the engine's stream; needs no
 * smr_results_fetch and leaves the host copy alone; changes no stored state; may be repeated and gives the same bytes.  Device memory: that of
 * smr_rows_part, shared with it. */
int smr_pairwise_part(smr_ctx*, int slot, const smr_params*, const smr_index* ix, double lambda, double K, uint64_t full_ref_corr, uint64_t full_read_corr,
                      uint8_t* bytes, uint64_t cap, uint64_t* need);
/* HIP-event milliseconds of the last smr_pairwise_part: {guards / statistics, sizes and scans, write, bytes D2H} (the last two 0 for a size-only call) */
int smr_pairwise_times(const smr_ctx*, double ms[4]);
/* The members of otu_map.txt (-otu_map) of the selected batch for ONE (index, part), found, grouped and written on the device (csrc/smr_otu.hpp):
 * what smr_results_fetch + smr_reads_record_text + smr_result_record + smr_report_add leave in the report's map entries of that key one read at
 * a time ("Writing the OTU map and aligned_denovo.* from the device").  Call it after smr_idcov_part has run for every (index,
 * part) of the run, once per (index, part) with that part resident in `slot`; slot, params and ix as for smr_rows_part.  As the host writer
 * (fill_otu_map2, otumap.cpp:131-198) it classifies AGAIN every stored alignment of the key of every read whose c_yid_ycov > 0, over the
 * FORWARD read letters whatever the strand, rounding with `floor(x * 1000.0 + 0.5) * 0.001` (not `/ 1000.0` as the pass does: 9 * 0.001 >
 * 9 / 1000.0); an alignment that passes both thresholds adds the read's id (the header up to the first space, without '>' / '@') to the group
 * of its reference.  Groups come in ascending ref_num, the members of a group in read order, then alignment-slot order; the text of group g is
 * bytes[groups[g].off, groups[g + 1].off or need[0]): its ids joined by '\t', no terminator; groups lie back to back.  *any_yid_ycov: does any
 * read of the batch have c_yid_ycov > 0 -- whether the map file exists at all, whatever passed for this key.
 *   bytes / groups  either NULL: sizes only.  cap < need[0] or groups_cap < need[1]: SMR_ERR_CAPACITY, need valid, nothing written.  Otherwise
 *                   exactly need[0] bytes and need[1] groups are written and nothing behind them is touched.  `bytes` may be pinned memory.
 * SMR_ERR_STATE: a batch without kept text (the message names SMR_FASTX_KEEP); for a read with c_yid_ycov > 0, an alignment of the key without
 * a CIGAR.  SMR_ERR_ARG: thresholds outside [0, 1] or NaN; `ix` is not the part in `slot`; and -- for reads with c_yid_ycov > 0, counted on the
 * device before any byte is written -- a CIGAR with an M column outside its read or its reference (what the host writer refuses; insertions or deletions
 * that alone run past the end are accepted as there), a negative read_begin1 / ref_begin1, ref_num >= the part's references.  A batch on which the
 * pass never ran gives zero groups and *any_yid_ycov = 0.  Every refusal leaves a message that names the call, writes nothing and leaves the
 * context usable.  Runs on the engine's stream; needs no smr_results_fetch; changes no stored state (it sets no mark as smr_idcov_part does);
 * may be repeated and gives the same bytes.  Device memory, kept for the next call: 1 byte per alignment slot, 24 per read, 32 per member,
 * 2 KB per 1024 members, the output. */
typedef struct { uint32_t ref_num, n_reads; uint64_t off; } smr_otu_group;
int smr_otu_part(smr_ctx*, int slot, const smr_params*, const smr_index* ix, double min_id, double min_cov,
                 uint8_t* bytes, uint64_t cap, smr_otu_group* groups, uint64_t groups_cap, uint64_t need[2] /* bytes, groups */, int* any_yid_ycov);
/* HIP-event milliseconds of the last smr_otu_part or smr_otu_part_mates: {classify, sizes and scans, sort, write, D2H} (the last two 0 for a sizes-only call) */
int smr_otu_times(const smr_ctx*, double ms[5]);
/* smr_otu_part for mates that were read from two files (csrc/smr_otu_mates.hpp; INTEGRATION.md, "The OTU map of two-file mates from the
 * device"): read i of the selected batch is mate 1 of pair i, read i of batch `mates` its mate 2, as in smr_rows_part_mates and layout 2 of
 * smr_fastx_split.  Call it after smr_idcov_part has run for every (index, part) on BOTH batches.  The result is what the add_otu calls inside
 * smr_report_add_pair(pair 0), (pair 1), ... leave in the report's map entries of the key: groups ascend by ref_num; inside a group the members
 * stand in pair order, mate 1 before mate 2, then alignment-slot order; each mate is judged by its own c_yid_ycov and its id comes from its own
 * batch's kept text.  Group text, table, rounding, forward letters and id rule are those of smr_otu_part.  *any_yid_ycov: does any read of
 * either batch have c_yid_ycov > 0.  The arguments behind `mates` and the bytes / groups / cap / need contract are smr_otu_part's.  Two empty
 * batches, or two batches on which the pass never ran: SMR_OK with zeros (a batch without the pass has no members).
 * Refusals, in this precedence: (1) SMR_ERR_ARG: a NULL, a slot outside 0..63, `mates` outside 0..15 or the selected batch, thresholds outside
 * [0, 1] or NaN; (2) every refusal of smr_otu_part for the selected batch, its device-side guards included; (3) SMR_ERR_STATE: batch `mates`
 * holds no reads or not their text (the message names SMR_FASTX_KEEP and the batch); (4) SMR_ERR_ARG: unequal read counts, FASTA against FASTQ;
 * (5) the device-side guards of smr_otu_part for batch `mates` (the message names the batch).  SMR_ERR_CAPACITY: 2^31 reads or more in a batch,
 * 2^32 members or more over both.  Every message names the call; nothing is written and the context stays usable.  Changes no stored state,
 * selects no batch, may be repeated and gives the same bytes.  Device memory, kept and grown only: that of smr_otu_part (shared with it), its
 * per-read part (1 byte per alignment slot, 24 per read) once more for the mates' batch, 32 bytes per member of both batches. */
int smr_otu_part_mates(smr_ctx*, int mates, int slot, const smr_params*, const smr_index* ix, double min_id, double min_cov,
                       uint8_t* bytes, uint64_t cap, smr_otu_group* groups, uint64_t groups_cap, uint64_t need[2] /* bytes, groups */, int* any_yid_ycov);
/* HIP-event milliseconds of the last smr_otu_part_mates: {classify, size + scan of the selected batch; classify, size + scan of batch `mates`;
 * the merged compaction (k_otu_mates_pairs)}; all 0 when the last call was smr_otu_part.  smr_otu_times reports the last call of either form
 * (for this one: both classify stages; both size stages, the compaction and the sizes of the text; sort; write; D2H). */
int smr_otu_mates_times(const smr_ctx*, double ms[5]);
/* Test seam of the sort of smr_otu_part: perm[0..n) = the STABLE permutation that orders keys[] (each below 2^key_bits, key_bits <= 32:
 * SMR_ERR_ARG otherwise) ascending -- ceil(key_bits / 8) radix passes, none for key_bits = 0. */
int smr_otu_sort_batch(smr_ctx*, uint32_t n, const uint32_t* keys, uint32_t key_bits, uint32_t* perm);
/* The aligned_denovo.* FASTX outputs (-de_novo_otu) of the selected batch, written on the device beside smr_fastx_split, whose layouts, `mates`
 * and size / capacity / state contract it shares (want_aligned / want_other are ignored).  Four streams; stream j is bytes[off[j], off[j + 1]),
 * off[4] = *need, and belongs to the aligned_denovo file smr_report_open gives index j.  A read is a de novo read when n_denovo > 0 and the other
 * three counters of smr_idcov_part are 0 (a batch without the pass has none) -- or, with `dn`, when its byte there is non-zero (the reads of the
 * selected batch, then, layout 2, those of batch `mates`).  Layout 0 routes as smr_report_add, layouts 1 and 2 by the table of
 * smr_report_add_pair (ReportDenovo::append, report_denovo.cpp:57-134), its two quirks under out2 included: nothing for a pair under paired_out
 * unless both mates are de novo reads, and otherwise BOTH mates written, the one that is no de novo read to file 0. */
int smr_fastx_denovo(smr_ctx*, int mates, const smr_fxsplit_opts*, const uint8_t* dn /* NULL: the batches' own counters */,
                     uint8_t* bytes, uint64_t cap, uint64_t off[5], uint64_t* need);

/* ---- gzip on the device ----------------------------------------------------------------------------------------------------------------
 * A DEFLATE compressor in HIP kernels.  A byte range (a "stream") is cut into chunks of smr_gzip_chunk() plain bytes, the last one may be
 * shorter, and every chunk becomes one complete gzip member: a 10-byte header (mtime 0, no name), dynamic-Huffman DEFLATE data whose
 * back-references stay inside the chunk (or stored blocks where coding would not make the member smaller), CRC-32 and ISIZE, both computed
 * on the device.  The members of a stream lie back to back -- a multi-member gzip file, as the reference's merged per-thread outputs are;
 * an empty stream gives no byte.  The same bytes in give the same bytes out, whatever else is in the call.
 * smr_gzip_bound: no output for plain_bytes in n_chunks members is larger -- per member 18 + its plain bytes + 5 per stored block of at most
 * 65 535 bytes; for the ceil(len / chunk) members of one stream of len bytes the value is exactly that sum. */
uint32_t smr_gzip_chunk(void);
uint64_t smr_gzip_bound(uint64_t plain_bytes, uint64_t n_chunks);
/* A building block and the test seam: stream k is plain[off[k], off[k + 1]) of a HOST buffer (off ascending, n_streams + 1 entries); its
 * members are gz[gz_off[k], gz_off[k + 1]), gz_off[n_streams] = *need.  gz == NULL: the sizes only (this costs the matching and the code
 * building, i.e. most of a compression: with smr_gzip_bound one call is enough).  cap < *need: SMR_ERR_CAPACITY, gz_off and *need valid,
 * nothing written.  Otherwise exactly *need bytes are written.  gz may be pinned memory. */
int smr_gzip_batch(smr_ctx*, const uint8_t* plain, const uint64_t* off /* n_streams + 1 */, uint32_t n_streams,
                   uint8_t* gz, uint64_t cap, uint64_t* gz_off /* n_streams + 1 */, uint64_t* need);
/* smr_fastx_split / smr_fastx_denovo whose streams stay on the device and cross the bus as gzip members: the same measure, scan and copy
 * kernels, then the compressor on the engine's stream.  Routing, layouts, `hit` / `dn`, refusals and the state contract are the plain
 * calls'; plain_off is what the plain call returns in `off`; stream k is gz[gz_off[k], gz_off[k + 1]), the last offset = *need, an empty
 * stream has no byte.  gz == NULL: sizes only (a full compression but for the bit packing); cap < *need: SMR_ERR_CAPACITY with the offsets and
 * *need valid and nothing written; otherwise exactly *need bytes.  The calls change no stored state and may be repeated: the same bytes. */
int smr_fastx_split_gz(smr_ctx*, int mates, const smr_fxsplit_opts*, const uint8_t* hit,
                       uint8_t* gz, uint64_t cap, uint64_t gz_off[9], uint64_t plain_off[9], uint64_t* need);
int smr_fastx_denovo_gz(smr_ctx*, int mates, const smr_fxsplit_opts*, const uint8_t* dn,
                        uint8_t* gz, uint64_t cap, uint64_t gz_off[5], uint64_t plain_off[5], uint64_t* need);
/* The same compressor with members that end at line ends, for text made of rows.  Nominal cuts lie every 48 KiB (the pitch) of a stream; each
 * is moved back to behind the last '\n' of the 16 KiB (the window) in front of it, and stays where it is when the window holds none: a line
 * longer than 16 KiB is cut wherever the grid falls, which is no error.  A stream of n bytes gives ceil(n / pitch) members of at most 64 KiB -
 * 1 plain bytes each; any prefix of the members of a text whose lines are shorter than the window inflates to whole lines.  Every cut is a
 * function of the text alone (a kernel on a fixed grid, csrc/smr_gzip.hpp), so the output is as deterministic as smr_gzip_batch's.
 * smr_gzip_lines_bound: no output for plain_bytes in n_streams streams is larger (smr_gzip_bound of plain_bytes / pitch + n_streams members).
 * smr_gzip_lines_batch: the contract of smr_gzip_batch, argument for argument. */
uint64_t smr_gzip_lines_bound(uint64_t plain_bytes, uint32_t n_streams);
int smr_gzip_lines_batch(smr_ctx*, const uint8_t* plain, const uint64_t* off /* n_streams + 1 */, uint32_t n_streams,
                         uint8_t* gz, uint64_t cap, uint64_t* gz_off /* n_streams + 1 */, uint64_t* need);
/* smr_rows_part / smr_pairwise_part whose text stays on the device and crosses the bus as gzip members cut at line ends: the same guard, size
 * and write kernels, then the compressor on the engine's stream.  Arguments, guards, refusals (their messages name the _gz call), call order
 * and the state contract are the plain calls'; plain_off / *plain_bytes is what the plain call returns in off / *need.  Stream k (SAM rows,
 * BLAST rows) is gz[gz_off[k], gz_off[k + 1]), gz_off[2] = *need; of smr_pairwise_part_gz the members are gz[0, *need).  A stream that is not
 * wanted or holds no row has no byte.  gz == NULL: sizes only (the text is written and compressed but for the bit packing); cap < *need:
 * SMR_ERR_CAPACITY with the offsets and *need valid and nothing written; otherwise exactly *need bytes, at most smr_gzip_lines_bound(plain
 * bytes, streams).  The calls change no stored state and may be repeated: the same bytes.  smr_rows_times / smr_pairwise_times then report
 * 0 for the copy that was not made; smr_gzip_times has the compressor's share. */
int smr_rows_part_gz(smr_ctx*, int slot, const smr_params*, const smr_index* ix, const smr_rows_opts*,
                     uint8_t* gz, uint64_t cap, uint64_t gz_off[3], uint64_t plain_off[3], uint64_t* need);
int smr_pairwise_part_gz(smr_ctx*, int slot, const smr_params*, const smr_index* ix, double lambda, double K, uint64_t full_ref_corr, uint64_t full_read_corr,
                         uint8_t* gz, uint64_t cap, uint64_t* plain_bytes, uint64_t* need);
/* HIP-event milliseconds of the compressor in the last of the calls above: {matching + CRC (with the line cuts, where there are any), code
 * building, bit packing, scan + compaction, bytes D2H} (the last three 0 for a sizes-only call) */
int smr_gzip_times(const smr_ctx*, double ms[5]);

/* ---- the reports of mates in two reads files, written on the device (csrc/smr_mates.hpp, csrc/smr_engine_mates.hpp) ----
 * smr_rows_part, smr_pairwise_part and their _gz forms for a paired run whose mates were read from two files: read i of the SELECTED batch is
 * mate 1 of pair i, read i of batch `mates` its mate 2 (the layout 2 of smr_fastx_split).  Each stream holds exactly what the host writer
 * appends for that (index, part) when it is fed smr_report_add_pair(pair 0), (pair 1), ...: the rows of mate 1 of pair 0, of mate 2 of pair 0,
 * of mate 1 of pair 1, and so on -- no OTU or FASTX output, which have their own calls.  The guard, size and write kernels are the plain
 * calls', run over the selected batch and then over batch `mates`; a further kernel (k_mates_zip) interleaves the two staged outputs on the
 * device: with a[i] / b[i] the byte offsets of read i in the two batches' streams, the rows of mate 1 of pair i go to a[i] + b[i] and those
 * of mate 2 to a[i + 1] + b[i].  smr_report_add_rows, smr_report_add_pairwise and their _gz forms take the bytes as they are.
 * The contract is the sibling's, argument for argument: bytes == NULL: sizes only (the guard and size stages of the two batches and nothing
 * else); cap < *need: SMR_ERR_CAPACITY with the offsets and *need valid and nothing written; otherwise exactly *need bytes and nothing behind
 * them.  `bytes` may be pinned.  No stored state changes, the selected batch stays selected on every path, and a repeated call gives the same
 * bytes.  The _gz forms return what smr_rows_part_gz / smr_pairwise_part_gz return, made of the interleaved text (the members smr_gzip_lines_batch
 * makes of the plain _mates bytes).
 * Refusals, in their precedence (every message names the _mates call made; afterwards the context is usable and nothing is written):
 *   1. SMR_ERR_ARG: a NULL argument, a slot outside 0..63, `mates` outside 0..15 or the selected batch itself;
 *   2. every refusal of the plain call for the selected batch, its device-side guards included;
 *   3. SMR_ERR_STATE: batch `mates` holds no reads or not their text (SMR_FASTX_KEEP); the message names the batch;
 *   4. SMR_ERR_ARG: the two batches differ in their number of reads, or one is FASTA and the other FASTQ (the words of smr_fastx_split);
 *   5. the plain call's device-side guards for batch `mates` (a CIGAR missing, without columns, or past its read or reference; ref_num; a score
 *      beyond the table); the message names the batch.
 * Two empty batches: SMR_OK with zeros.
 * Device memory, kept and grown only: the plain call's, the same once more for the mates' batch, and the interleaved output (the bytes of both
 * batches plus an eighth).  The e-value table (sized for the longer max_len of the two batches) and the slot's reference names are shared. */
int smr_rows_part_mates(smr_ctx*, int mates, int slot, const smr_params*, const smr_index* ix, const smr_rows_opts*,
                        uint8_t* bytes, uint64_t cap, uint64_t off[3], uint64_t* need);
int smr_pairwise_part_mates(smr_ctx*, int mates, int slot, const smr_params*, const smr_index* ix, double lambda, double K,
                            uint64_t full_ref_corr, uint64_t full_read_corr, uint8_t* bytes, uint64_t cap, uint64_t* need);
int smr_rows_part_mates_gz(smr_ctx*, int mates, int slot, const smr_params*, const smr_index* ix, const smr_rows_opts*,
                           uint8_t* gz, uint64_t cap, uint64_t gz_off[3], uint64_t plain_off[3], uint64_t* need);
int smr_pairwise_part_mates_gz(smr_ctx*, int mates, int slot, const smr_params*, const smr_index* ix, double lambda, double K,
                               uint64_t full_ref_corr, uint64_t full_read_corr, uint8_t* gz, uint64_t cap,
                               uint64_t* plain_bytes, uint64_t* need);
/* The interleave kernel at its seam (a test seam and a building block): piece i of A is a[a_off[i], a_off[i + 1]), likewise B; HOST buffers,
 * n + 1 ascending offsets each.  out takes piece 0 of A, piece 0 of B, piece 1 of A, ...: *need = the bytes of all pieces.  n == 0: SMR_OK;
 * offsets that decrease: SMR_ERR_ARG; out == NULL: the size only; cap < *need: SMR_ERR_CAPACITY with *need valid and nothing written;
 * otherwise exactly *need bytes and nothing behind them. */
int smr_interleave_batch(smr_ctx*, uint32_t n, const uint8_t* a, const uint64_t* a_off, const uint8_t* b, const uint64_t* b_off,
                         uint8_t* out, uint64_t cap, uint64_t* need);
/* HIP-event milliseconds of the last *_mates call: {the selected batch's stages, the mates' stages, the interleave, bytes D2H (0 for a
 * sizes-only call and for the _gz forms)} */
int smr_mates_times(const smr_ctx*, double ms[4]);

/* ---- gunzip on the device --------------------------------------------------------------------------------------------------------------
 * A DEFLATE decoder in HIP kernels (csrc/smr_gunzip.hpp): a gzip file of any number of members, inflated by many waves at once.  The starts of
 * non-final dynamic-Huffman blocks and of members are found speculatively; tasks at least `grain` compressed bytes apart (1: every candidate;
 * 0: the default, 65 536, and 1 for a file of fewer than 4 096 candidates) are decoded with the 32 KiB in front of each as placeholders,
 * stitched in file order, and the placeholders resolved;
 * CRC-32 and ISIZE of every member are checked.  The host inflate (zlib) stays the definition of every answer and every refusal: whatever the
 * device does not settle -- a decode error, a CRC-32 or ISIZE mismatch, a truncated file, bytes behind the last member, more stitching rounds
 * than the build allows -- is inflated by zlib in the same call, whose result, or error code (SMR_ERR_IO) and message, is then the call's.
 * smr_gunzip_batch: the n bytes at gz (HOST memory) -> plain.  plain == NULL: the size only.  cap < *need: SMR_ERR_CAPACITY, *need valid,
 * nothing written.  Otherwise exactly *need bytes are written.  The call changes no stored state and may be repeated: the same bytes. */
int smr_gunzip_batch(smr_ctx*, const uint8_t* gz, uint64_t n, uint64_t grain /* 0 = default */, uint8_t* plain, uint64_t cap, uint64_t* need);
/* Of the last smr_gunzip_batch / inflating smr_reads_upload_fastx*:
 *   info[0]  path | why << 8 | rounds << 16.  path 0: the device, 1: the host.  why: 0 -, 1 not a file the device takes (shorter than 18
 *            bytes, 2^38 bytes or more, no member header at byte 0, more than 16 MiB per candidate or 64 MiB in one piece -- serial work
 *            for one wave --, text beyond the caller's limit), 2 more candidates than the list holds, 3 rounds exhausted, 4 a decode
 *            error, 5 a distance too far back, 6 a CRC-32 or ISIZE mismatch, 7 truncated, 8 bytes behind the last member, 9 a header CRC
 *            mismatch.  rounds: counting passes run (1: every end hit a task start)
 *   info[1]  candidates found        info[2]  tasks (on the device path: the confirmed ones)        info[3]  members
 *   info[4]  stored blocks | fixed blocks << 32        info[5]  dynamic blocks        info[6]  compressed bytes        info[7]  plain bytes */
int smr_gunzip_info(const smr_ctx*, uint64_t info[8]);
/* HIP-event milliseconds of the last such call on the device path: {H2D, find, count, write, window, resolve + CRC} (0 on the host path) */
int smr_gunzip_times(const smr_ctx*, double ms[6]);
/* A TEST SEAM, not part of the stable interface (it may change or go with the decoder's inner workings; tests/helpers/gunzipdev.py compares
 * the starts with a model's): the confirmed tasks of the last such call on the device path, in file order: start bit << 2 | 2 (not a candidate of the
 * search: made by the stitch from a predecessor's end) | 1 (starts at a member header; else at a block header).  starts may be NULL;
 * at most cap entries are written, *count is the number of tasks. */
int smr_gunzip_tasks(const smr_ctx*, uint64_t* starts, uint64_t cap, uint64_t* count);
/* Forget all per-read results/counters of the resident batch (reads stay resident). */
int smr_state_reset(smr_ctx*);

/* The hot path for ONE (index, part) over the resident batch: both strands, all passes, LIS chaining,
 * Smith-Waterman scoring; commits per-read state exactly like processor.cpp:104-161 + kvdb.put.
 * Synchronous (returns after the GPU finished). */
int smr_align_part(smr_ctx*, int slot, const smr_params*);
/* Banded traceback -> CIGAR for every stored alignment that does not have one yet and whose
 * (index_num, part) is resident in `slot` (ssw.c:577-773).  Call after smr_align_part of that slot. */
int smr_traceback(smr_ctx*, int slot, const smr_params*);

/* Readstats counters (readstats.hpp:77-85): out[0]=num_aligned, out[1]=num_short (of the last part),
 * out[2+i]=reads_matched_per_db[i], i < n_db.  These are what the RCCL all-reduce sums across ranks. */
int smr_counters(smr_ctx*, uint64_t* out, uint32_t n_db);
/* Device pointer + count of the u64 counters block (for an in-place RCCL all-reduce by the caller). */
int smr_counters_device(smr_ctx*, void** dptr, uint32_t* n_u64);
/* d_acc[k] += counter k of the selected batch for k < n_u64 (<= the count smr_counters_device gives, or <= SMR_COUNTERS_WITH_IDCOV: k = 66 .. 69 are
 * the four sums of smr_idcov_counters), on the device: a host that aligns its shard chunk by chunk through a few recycled batches keeps one device
 * block of sums (and all-reduces THAT over the ranks). */
int smr_counters_accumulate(smr_ctx*, void* d_acc, uint32_t n_u64);

/* ------------------------------------------------------------------------------------------------
 * %id / %coverage pass (the reference's denovo_stats, processor.cpp:287-438: what -otu_map and -de_novo_otu need).
 * Call order: smr_align_part + smr_traceback for EVERY (index, part) of the run, then smr_idcov_part once per (index, part) with that part's
 * references resident in `slot`, then smr_results_fetch.  The reference runs the pass after all alignment; here smr_align_part answers
 * SMR_ERR_STATE once the pass has counted an alignment of the batch (smr_state_reset / smr_reads_upload* start over; a call that found no
 * alignment to count changes nothing).  A host that keeps one slot and uploads part after part therefore uploads every part a second time
 * for the pass when there is more than one; keeping the parts resident in slots 0..63 avoids that.
 * ---------------------------------------------------------------------------------------------- */
/* denovo_stats for ONE (index, part): processor.cpp:287-366.  Every stored alignment of that part is walked along its CIGAR over the read and
 * the reference letters (n_miss, n_gap, n_match of Read::calc_miss_gap_match), id = n_match / (n_miss + n_gap + n_match) and
 * cov = |read_end1 - read_begin1 + 1| / readlen are rounded to three decimals and compared with min_id / min_cov (each within [0, 1], else SMR_ERR_ARG);
 * the class (both / id only / coverage only / neither) bumps one of the read's four counters (Read::c_yid_ycov, n_yid_ncov, n_nid_ycov, n_denovo:
 * smr_result_record writes them; zero without this call) and one of the batch's.  Like the reference, the walk reads the FORWARD read also for an
 * alignment on the reverse strand (csrc/smr_idcov.hpp says why).  SMR_ERR_STATE when an alignment of the part has no CIGAR yet.  Each alignment is
 * counted once: a second call for the same (index, part) changes nothing.  SMR_ERR_CAPACITY when reads x alignment slots reaches 2^32. */
int smr_idcov_part(smr_ctx*, int slot, const smr_params*, double min_id, double min_cov);
/* out = {n_yid_ycov, n_yid_ncov, n_nid_ycov, num_denovo} of the selected batch (readstats.hpp:77-85) */
int smr_idcov_counters(smr_ctx*, uint64_t out[4]);
/* Device pointer to those four u64 (for an in-place all-reduce by the caller; SMR_ERR_STATE when the selected batch has no counter block
 * yet); smr_counters_device keeps handing out its 66.
 * smr_counters_accumulate takes them as k = 66 .. 69 of a block of SMR_COUNTERS_WITH_IDCOV u64. */
int smr_idcov_counters_device(smr_ctx*, void** dptr, uint32_t* n_u64);
#define SMR_COUNTERS_WITH_IDCOV 70
/* The kernels of the pass at the seam of Read::calc_miss_gap_match: n independent triples (read i in the 0..4 alphabet, FORWARD letters, bytes
 * [read_off[i], read_off[i+1]); the reference window that starts at the alignment's first reference letter; BAM-style u32 CIGAR operations
 * length << 4 | op, op 0 / 1 / 2 = M / I / D, [cigar_off[i], cigar_off[i+1])) with read_begin / read_end / readlen as s_align2 carries them:
 * out[4 i ..] = {n_miss, n_gap, n_match, class} with class 0 = id and coverage, 1 = id only, 2 = coverage only, 3 = neither.
 * SMR_ERR_ARG when a CIGAR runs past its read or window. */
int smr_idcov_batch(smr_ctx*, uint32_t n, const uint8_t* reads, const uint64_t* read_off, const uint8_t* refs, const uint64_t* ref_off,
                    const uint32_t* cigars, const uint64_t* cigar_off, const int32_t* read_begin, const int32_t* read_end, const uint32_t* readlen,
                    double min_id, double min_cov, uint32_t* out);

/* Results.  smr_result_record writes Read::toBinString() bytes of read i (the KVDB value,
 * read.cpp:429-462; 0 bytes when the read has no alignment) and returns the size needed. */
int    smr_results_fetch(smr_ctx*);                       /* device -> host copy of all per-read results */
size_t smr_result_record(const smr_ctx*, uint32_t read_idx, uint8_t* buf, size_t cap);
/* The same for read i of batch `batch`, whichever batch is selected.  It only reads the host copy that smr_results_fetch made of that
 * batch, so a second host thread may serialise the records of batch k while the first one is aligning batch k+1 (the reference's writer
 * thread works the same way behind its aligners, output.cpp:169-272). */
size_t smr_result_record_batch(const smr_ctx*, int batch, uint32_t read_idx, uint8_t* buf, size_t cap);
int    smr_result_is_hit(const smr_ctx*, uint32_t read_idx);

/* Resuming a run (the reference restores every read from its key-value store at the start of every (index, part), Read::load_db, read.cpp:467-539,
 * skips the reads stored as done, processor.cpp:116-126, and so continues a run that an earlier process stopped after any part -- e.g. on further --ref files).
 * Inverse of smr_result_record for the selected batch.  bytes = the records back to back; off[0..n]:
 * record i is bytes[off[i], off[i+1]) and off[i] == off[i+1] means "read i has no stored record" (off[0] need not be 0: the offsets of a
 * chunk of reads within the records of a whole run serve as they are; only bytes[off[0], off[n]) are read).
 * n must equal the batch's read count.  Replaces the batch's whole stored state: a read without a record
 * gets the state of a fresh upload.  The bytes are copied to the device once and parsed there.
 * Call order: after smr_reads_upload[_batch] (or smr_state_reset, or any smr_align_part / smr_traceback, whose results it replaces) and before the first
 * smr_idcov_part that counted an alignment of the batch; otherwise SMR_ERR_STATE.  Afterwards smr_align_part, smr_traceback, smr_results_fetch and
 * smr_result_record behave as if this context had produced the state itself: a part continues from it, an alignment stored with its CIGAR keeps it, one
 * stored without (a record taken before smr_traceback) stays without, and smr_traceback of a later part touches only that part's alignments.  The
 * records' num_alignments field becomes what smr_result_record writes, so import -> fetch -> record is the identity.
 * Refused, each with a message, the batch left as an upload leaves it and the context usable: records whose lengths (alignment_size, an alignment's
 * length, a CIGAR length) do not add up to off[i+1] - off[i] -- cut short, trailing bytes -- SMR_ERR_ARG; more alignments in a record than
 * max_alignments_per_read SMR_ERR_CAPACITY; an alignment's readlen that is not the uploaded read's length SMR_ERR_ARG; a non-zero id / coverage counter
 * (a record taken after smr_idcov_part: resuming there is not supported) SMR_ERR_ARG; records that disagree on num_alignments SMR_ERR_ARG; n that is
 * not the batch's read count SMR_ERR_ARG.  Every field is checked against the end of its record before it is read: nothing beyond bytes + off[n] is touched.
 * NOT part of the stored state and not imported: the Readstats counters (smr_counters_import below sets them; smr_state_import leaves them alone, so the
 * two calls come in either order) and the work counters of smr_prof (n_hit, n_sw_fwd, ...), which count what THIS context did. */
int smr_state_import(smr_ctx*, const uint8_t* bytes, const uint64_t* off, uint32_t n);
/* The other direction: the records of the whole selected batch in one call, sized and serialised on the device (csrc/smr_export.hpp), back to back in
 * bytes with their offsets in off[0..n] (off[0] = 0; off[i] == off[i+1]: read i has no alignment and no record).  The (bytes, off) pair is what
 * smr_state_import takes and what a state file or a key-value writer wants.  Acts on the selected batch on the engine's stream (the threading rule of
 * smr_results_fetch, which it neither needs nor disturbs) and is allowed wherever smr_results_fetch is: before smr_traceback (CIGAR length 0), after it,
 * after smr_idcov_part (the four id / coverage counters are then the read's, else 0).  n must be the batch's read count, else SMR_ERR_ARG; without an
 * uploaded batch SMR_ERR_STATE.  off (n + 1 entries) and need may each be NULL; what is given is always filled, *need = off[n] = the bytes of all records.
 * bytes == NULL: sizes only.  cap < *need: SMR_ERR_CAPACITY, nothing is written to bytes, off and *need are valid.  Otherwise exactly *need bytes are
 * written and nothing at or behind bytes + *need is touched; bytes may be pinned memory.
 * Invariants: for every i, bytes[off[i], off[i+1]) is what smr_results_fetch + smr_result_record(i) give, byte for byte; and
 * smr_state_export -> smr_state_import restores the batch's stored state wherever smr_state_import accepts the records. */
int smr_state_export(smr_ctx*, uint8_t* bytes, uint64_t cap, uint64_t* off, uint32_t n, uint64_t* need);
/* Inverse of smr_counters: same layout, same n_db (<= 64; reads_matched_per_db beyond n_db become 0).  Same call order as smr_state_import. */
int smr_counters_import(smr_ctx*, const uint64_t* in, uint32_t n_db);

/* Seed hits of the last smr_seed_scan call (kernel-level parity + roofline bench of the seed-scan kernel).
 * Runs ONLY the window-scan/burst-trie kernel for (strand, pass) over every read of the resident batch. */
int smr_seed_scan(smr_ctx*, int slot, const smr_params*, int strand, int pass, uint64_t* n_hits_out);
/* hits as (read_idx, id, win) triples in unspecified order */
int smr_seed_hits_fetch(smr_ctx*, uint32_t* triples, uint64_t cap_triples, uint64_t* n_out);

/* Timing/work counters accumulated since the last smr_prof_reset (HIP events on the engine's stream). */
typedef struct {
  double   seed_ms;  uint64_t seed_launches;   /* window-scan + burst-trie kernel */
  double   chain_ms; uint64_t chain_launches;  /* LIS chaining + SW scoring kernel */
  double   trace_ms; uint64_t trace_launches;  /* banded traceback kernel */
  /* exact work counters of the seed-scan kernel (SURVEY.md 8d byte formula) */
  uint64_t n_windows, n_lookup, n_node, n_entry, n_hit, n_read_bytes;
  uint64_t n_sw_fwd, n_sw_rev, n_sw_cells;     /* ssw_align calls of the sequential walk (forward / reverse passes) and their DP cells */
  uint64_t n_sw_spec, n_sw_spec_used;          /* forward passes scored ahead of the walk in four-problem batches, and how many of them the walk then asked for */
  uint64_t n_seed_redo;                        /* waves (64 searches) of the fast seed kernel whose candidate pool overflowed and that the per-lane DFS kernel searched again */
  uint64_t hit_list_cap;                       /* entries of the per-search hit lists in use: 4, doubled on demand up to 128, then 31 L/2 - 20 (twice that for the DFS kernel) = what a search can accept at most */
  uint64_t n_seed_shared;                      /* seed stages since smr_prof_reset whose searches walked the batch's SHARED sorted arrays (one sort for several index parts / --ref) */
  uint64_t n_seed_shared_builds;               /* ... and how often those six arrays were built */
} smr_prof;
/* smr_index_build with the per-occurrence work (sorting all (L+1)-mers, ids, position lists, mini-trie layout) done
 * on the device: same arguments (threads does not apply), same smr_index objects, byte-identical index files
 * (replaces build_index, indexdb.cpp:1119-2095). */
int smr_index_build_gpu(smr_ctx*, const char* ref_fasta, uint32_t lnwin, double max_mb, uint32_t max_pos,
                        smr_index** parts_out, uint32_t cap_parts, uint32_t* n_parts_out, char* err, size_t errcap);

/* Device self-check: n_cases seeded random (read, reference window) pairs, 1..max_len nt, for two scoring schemes: the packed 16-bit
 * Smith-Waterman kernel against the 32-bit kernel (score, end cell; forward and reverse pass), both on the GPU.  smr_create runs it
 * (SMR_SW_SELFCHECK=<cases>, 0 = skip) and falls back to the 32-bit kernel if any case differs; SMR_SW_PACKED=0 disables the packed kernel,
 * SMR_SW_PACKED=2 selects its wave_ror variant (the kernel checked is the selected one). */
int smr_sw_selfcheck(smr_ctx*, uint32_t n_cases, uint32_t seed, uint32_t max_len, uint64_t* n_bad);
int smr_sw_mode(smr_ctx*, int set_to);
/* The candidate walk (alignment.cpp:150-508) runs in rounds of walk kernel -> Smith-Waterman over a task list -> next list; the last round scores inside
 * the walk kernel, so the records never depend on the number.  out[pass] = rounds the next smr_align_part runs for that pass: at most 8 (SMR_WALK_ROUNDS=<n>
 * fixes it), lowered part by part towards what the previous part needed (an empty round still costs three launches). */
int smr_walk_rounds(const smr_ctx*, uint32_t out[3]);
/* The SW kernels at the ssw.h seam: for n independent pairs (read / reference window in the 0..4 alphabet, pair i = bytes [off[i], off[i+1])),
 * what ssw_align(prof, ref, refLen, gapO, gapE, flag = 2, filters, 0, 0) returns without the CIGAR (ssw.h:118-140, ssw.c:834-941):
 * out[5 i ..] = {score1, ref_begin1, ref_end1, read_begin1, read_end1}, begins = -1 when score1 < filters (a pair without a positive cell: {0, -1, -1, -1, 0}, as ssw.c).  mode 0 / 1 / 2 = 32-bit / packed / packed wave_ror kernel, 3 = four pairs per wave (the fast kernels: only under the
 * schemes whose answers they share with ssw.c, SMR_ERR_ARG otherwise); mode 4 = the slow path that reproduces ssw.c's stripe geometry, any scheme;
 * mode 5 = the long-read strips (see smr_sw_long_rows below), a fast kernel like 0 - 3. */
int smr_ssw_batch(smr_ctx*, uint32_t n_pairs, const uint8_t* reads, const uint64_t* read_off, const uint8_t* refs, const uint64_t* ref_off,
                  int match, int mismatch, int score_N, int gap_open, int gap_ext, uint32_t filters, int mode, int32_t* out);   /* set_to 0 / 1: use the 32-bit / the packed kernel; other values: query; returns the mode in use */
/* mode 5 of smr_ssw_batch = what k_chain<LONG> and k_begins<LONG> call for the reads of a batch with long reads (sw_wave_any_t under the packed
 * wave_ror kernel): spans of more than 512 rows go through the strips of 128 virtual lanes x R rows, R = smr_sw_long_rows(m) in 8, 10 ... 24. */
int smr_sw_long_rows(int m);
/* The sixteen-problems-per-wave kernel k_sw16<rows> (smr_walk.hpp) at the same seam, launched as the candidate walk launches it: over the packed
 * records of the SELECTED batch (smr_reads_pack + smr_reads_upload) and a task list.  Task i scores rows [aq, aq + m) of read `read` (on its
 * reverse-complement strand when reversed = 1: row k is letter len - 1 - k, complemented) against ref[win_off, win_off + nref), `ref` (0..4
 * alphabet, ref_len bytes) standing in for the reference letters of an index part.  list_b = 0: the task goes to the list scored with end cells
 * and, when its score reaches `filters`, through the begin-cell pass (a second launch over tasks that run backwards from the end cell, as
 * k_begins_prep makes them): out[5 i ..] = {score1, ref_begin1, ref_end1, read_begin1, read_end1} as ssw_align returns them for the span and
 * the window (begins = -1 when score1 < filters).  list_b = 1: the score-only list, out[5 i ..] = {score1, -1, -1, -1, -1}.
 * rows = 13 / 19 / 26 / 32 (spans up to 8 x rows letters); blocks = 0: the grid the walk uses, else that many blocks (a small number = several
 * passes per block); force_any_n = 1: the kernel looks for ambiguous letters in every window even when `ref` has none.
 * SMR_ERR_ARG (with a message) for a task outside the kernel's stated range: m > 8 x rows or > 256, !sw_pk_fits, a scheme the fast kernels
 * do not take, rows outside the read, a window outside `ref`. */
typedef struct {
  uint32_t read, win_off;
  uint16_t aq, m, nref;
  uint8_t reversed, list_b;
} smr_sw16_task;
int smr_sw16_batch(smr_ctx*, uint32_t n_tasks, const smr_sw16_task* tasks, const uint8_t* ref, uint64_t ref_len, int force_any_n,
                   int match, int mismatch, int score_N, int gap_open, int gap_ext, uint32_t filters, int rows, uint32_t blocks, int32_t* out);
/* The PREFIX tasks of k_sw16 at the same seam (the kernel's third list): task i scores only the first `cols` columns of its window and returns an
 * interval that holds the score of the whole window: out[2 i ..] = {lo, hi}, lo = the best score over those columns, hi = max(lo, s min(m, rem),
 * max over the rows i < m of (best score of row i over those columns + s min(m - 1 - i, rem))) with rem = nref - cols and
 * s = max(match, mismatch, score_N, 0).  Everything else as smr_sw16_batch; SMR_ERR_ARG also for cols = 0, cols not a multiple of 4 (the kernel's
 * period of four columns) and cols >= nref. */
typedef struct {
  uint32_t read, win_off;
  uint16_t aq, m, nref, cols;
  uint8_t reversed, pad_[3];
} smr_sw16_prefix_task;
int smr_sw16_prefix_batch(smr_ctx*, uint32_t n_tasks, const smr_sw16_prefix_task* tasks, const uint8_t* ref, uint64_t ref_len, int force_any_n,
                          int match, int mismatch, int score_N, int gap_open, int gap_ext, int rows, uint32_t blocks, int32_t* out);
/* How the candidate walk uses prefix tasks, since smr_prof_reset.  Under best N (N > 0) a look-ahead task of a read that is expected to align is
 * scored over the first SMR_WALK_PREFIX per cent of its window's columns (default 44, 0 = off): the interval decides the task when it lies above
 * the minimal score, below the highest possible score and not above the lowest stored score of a read whose N slots are full -- the walk then
 * does with it what it does with every score inside; otherwise the task is scored again in full.  Records never depend on the switch.
 * out[0] prefix tasks scored, [1] consumed decisively, [2] met undecided and scored again, [3] never looked at; [4] / [5] the look-ahead tasks
 * (and their cells) of reads expected to align under best N, whatever the mode; [6] the switch as the context latched it; [7] 1 while the context leaves prefix tasks, 0 while it has stopped: after a part that met
 * fewer than two decided intervals per undecided one it leaves none for the next 64 parts, then tries again. */
int smr_walk_prefix_stats(smr_ctx*, uint64_t out[8]);
/* Launches of k_sw16<13 | 19 | 26 | 32> since smr_create: out[0..3] by the rounds of the candidate walk, out[4..7] by the begin-cell stage
 * (which instantiation a batch gets follows from its longest read; a batch that never takes the walk path counts nothing). */
int smr_sw16_launches(const smr_ctx*, uint64_t out[8]);
/* k_sw16h<R>: k_sw16<R> in packed f16 (v_pk_add_f16, v_pk_maximum3_f16: the three-operand maximum gfx950 lacks for 16-bit integers), bit-exact
 * because every value is an integer f16 holds.  Launched instead of k_sw16<R> (walk rounds, begin-cell stage, smr_sw16_batch,
 * smr_sw16_prefix_batch; smr_sw16_launches counts both) where the scheme allows it: match, mismatch and score_N + gap_open each an integer of
 * at most three significant bits (0..8, 10, 12, 14, 16, 20, ...: one table byte), and 8 R x match + gap_open + gap_ext + the largest of them <= 2048.
 * smr_create compares the two kernels on the device and keeps k_sw16 alone if they differ; SMR_SW16_F16=0 does the same by hand.
 * set_to: 0 / 1 = select, anything else = query only; returns the mode in use.  *launches (may be NULL): k_sw16h launches since smr_create. */
int smr_sw16_f16(smr_ctx*, int set_to, uint64_t* launches);
/* The traceback kernels at the same seam: for n independent triples (read window, reference window -- both exactly the aligned spans
 * [begin1, end1] -- and the alignment's score1) the CIGAR that banded_sw returns for them (ssw.c:577-773 as called from ssw_align,
 * ssw.c:919-926): BAM-style u32 operations (length << 4 | op, op 0/1/2 = M/I/D), pair i at cigar_out[cigar_off_out[i] .. cigar_off_out[i+1]).
 * Operations beyond cigar_cap are counted but not written.  Uses the same host logic and kernels as smr_traceback. */
int smr_cigar_batch(smr_ctx*, uint32_t n_pairs, const uint8_t* reads, const uint64_t* read_off, const uint8_t* refs, const uint64_t* ref_off,
                    const uint16_t* scores, int match, int mismatch, int score_N, int gap_open, int gap_ext,
                    uint32_t* cigar_out, uint64_t cigar_cap, uint64_t* cigar_off_out);
int smr_prof_reset(smr_ctx*);
int smr_prof_get(smr_ctx*, smr_prof* out);
/* The same period per kernel family (k_seed_keys, the tuple sort, k_seed_pg<0>, k_seed_pg<1>, k_seed_finish, k_cand, k_chain, k_begins,
 * k_trace, ..., k_idcov): HIP-event time on the engine's stream, number of launches, and for the seed-stage kernels the ALGORITHMIC HBM bytes of what
 * the shipped kernels themselves do, from exact device counters: every tuple (12 B) written once by k_seed_keys next to its inputs
 * (read records, per-read state, two lookup words per window), read and written once by each of the two sort passes, read once by
 * k_seed_pg, which adds per search 8 B of block table, its directory words, 4 B per string looked at, 8 B per accepted {rank, id} and
 * the hit-segment words it reads and writes; k_seed_finish the segment words it gathers.  bytes = 0 where nothing is counted.
 * This -- not the traversal of the reference, which k_seed_pg does not perform -- is the numerator of bench.py's roofline. */
typedef struct { char name[32]; double ms; uint64_t launches; uint64_t bytes; } smr_kprof;
int smr_prof_kernels(smr_ctx*, smr_kprof* out, uint32_t cap, uint32_t* n_out);

/* ------------------------------------------------------------------------------------------------
 * Reports (host side): the reference's second pass over reads + KVDB (writeReports, output.cpp:169-272), fed by
 * smr_result_record.  Files in out_dir: aligned.fa|fq, other.fa|fq (report_fx_base.cpp:176-205), aligned.blast = BLAST tabular m8
 * with the optional columns of `-blast '1 cigar qcov qstrand'` (report_blast.cpp:253-354), aligned.sam (report_sam.cpp:64-152).
 * Rows are written per (index, part) in --ref order, within a part in the order the reads were added, like the reference's loop.
 * ---------------------------------------------------------------------------------------------- */
typedef struct smr_report smr_report;
typedef struct {
  int fastx;             /* -fastx   aligned.fa|fq */
  int other;             /* -other   other.fa|fq   */
  int blast_tabular;     /* -blast 1 ...           */
  char blast_cols[64];   /* optional BLAST columns, space separated, in output order: "cigar", "qcov", "qstrand" */
  int sam;               /* -sam                   */
  int blast_pairwise;    /* -blast 0: the BLAST-like pairwise text (report_blast.cpp:130-252) instead of tabular rows */
  int sam_sq;            /* -SQ: @SQ lines of every reference sequence in the SAM header (report_sam.cpp:155-211) */
  /* paired reads (two read files, or -paired_in / -paired_out): smr_report_add_pair routes the two mates like ReportFastx::append /
   * ReportFxOther::append (report_fastx.cpp:57-133, report_fx_other.cpp:49-113) */
  int paired_in;         /* -paired_in: a pair with one aligned mate goes to aligned.* entirely  */
  int paired_out;        /* -paired_out: ... goes to other.* entirely                              */
  int out2;              /* -out2: separate files for the mates: *_fwd / *_rev                     */
  int sout;              /* -sout: separate files for pairs and singletons: *_paired / *_singleton */
  int zip_out;           /* gzip every report file, names + ".gz" (the reference does so for gzip reads files or -zip-out 1, report_fx_base.cpp:94-95) */
  /* the outputs of the %id / %coverage pass: the records must come from a run of smr_idcov_part with the same thresholds */
  int otu_map;           /* -otu_map: otu_map.txt, written by smr_report_close (fill_otu_map, otumap.cpp:131-281): one line per reference id that a read
                            with c_yid_ycov > 0 aligned to with %id >= min_id and %coverage >= min_cov -- id, then the read ids, tab separated; lines in
                            std::map order of the id, reads in (index, part) then input order; no file when no read passed (otumap.cpp:200,276) */
  int denovo;            /* -de_novo_otu: aligned_denovo.fa|fq (+ the _fwd / _paired ... suffixes, + .gz): the reads with n_denovo > 0 and the other
                            three counters 0 (output.cpp:133-143), mates routed like ReportDenovo::append (report_denovo.cpp:57-134) */
  double min_id, min_cov; /* -id / -coverage */
} smr_report_opts;
int smr_report_open(const char* out_dir, const smr_report_opts*, int is_fastq, smr_report** out, char* err, size_t errcap);
/* per --ref: Gumbel parameters and the corrected sizes (smr_refstats_corrected); per (index, part): where its reference ids/sequences are */
int smr_report_set_db(smr_report*, uint32_t index_num, double lambda, double K, uint64_t full_ref_corr, uint64_t full_read_corr);
int smr_report_set_part(smr_report*, uint32_t index_num, uint32_t part, const smr_index*);
/* one read: its header line as in the file (with '>' / '@'), letters, quality (NULL for FASTA), and its record (NULL, 0: none) */
int smr_report_add(smr_report*, const char* header, const char* seq, const char* qual, const uint8_t* record, size_t record_len);
/* a pair of mates (read i of the first and of the second file / two consecutive records of an interleaved file) */
int smr_report_add_pair(smr_report*, const char* header1, const char* seq1, const char* qual1, const uint8_t* record1, size_t record1_len,
                        const char* header2, const char* seq2, const char* qual2, const uint8_t* record2, size_t record2_len);
/* The streams of smr_fastx_split: stream k is appended to the open aligned.* (k < 4) / other.* (k - 4) file of that index, through gzip under
 * zip_out.  SMR_ERR_ARG, and nothing is written, when a stream that is not empty has no open file. */
int smr_report_add_fastx(smr_report*, const uint8_t* bytes, const uint64_t off[9]);
/* The streams of smr_rows_part for (index_num, part): appended to the report's SAM / BLAST rows of that key, so that smr_report_close writes the
 * files as ever.  SMR_ERR_ARG, and nothing is appended, when a stream that is not empty belongs to a report not opened for it (sam /
 * blast_tabular), when the offsets decrease, or when the (index, part) was not registered with smr_report_set_part. */
int smr_report_add_rows(smr_report*, uint32_t index_num, uint32_t part, const uint8_t* bytes, const uint64_t off[3]);
/* on != 0: smr_report_add / smr_report_add_pair leave the SAM and BLAST tabular rows alone (smr_report_add_rows brings them); FASTX, the OTU
 * map, aligned_denovo.* and BLAST pairwise are unaffected */
int smr_report_skip_rows(smr_report*, int on);
/* The stream of smr_pairwise_part for (index_num, part): its n bytes are appended to the report's BLAST text of that key, so that
 * smr_report_close writes aligned.blast as ever (through gzip under zip_out).  SMR_ERR_ARG, and nothing is appended, for a stream that is not
 * empty when the report was not opened with blast_pairwise, when it was opened with blast_tabular as well (the host writes no pairwise text
 * then), or when the (index, part) was not registered with smr_report_set_part. */
int smr_report_add_pairwise(smr_report*, uint32_t index_num, uint32_t part, const uint8_t* bytes, uint64_t n);
/* on != 0: smr_report_add / smr_report_add_pair leave the BLAST pairwise text alone (smr_report_add_pairwise brings it); FASTX, SAM, BLAST
 * tabular rows, the OTU map and aligned_denovo.* are unaffected */
int smr_report_skip_pairwise(smr_report*, int on);
/* on != 0: smr_report_add / smr_report_add_pair leave aligned.* / other.* alone (smr_report_add_fastx writes them); BLAST, SAM, the OTU map and
 * aligned_denovo.* are unaffected */
int smr_report_skip_fastx(smr_report*, int on);
/* The groups of smr_otu_part for (index_num, part): appended to the report's map entries of that key, behind what the key already holds; the
 * reference id of a group is sq_header[first_seq + ref_num], "*" beyond the table, as smr_report_add finds it.  Afterwards smr_report_close,
 * smr_report_otu_merge and smr_report_otu_count give the file, the merge and the count they would give had the same reads gone through
 * smr_report_add.  any_yid_ycov != 0: the map file exists.  SMR_ERR_ARG, and nothing is appended, when the report was opened without otu_map,
 * when the (index, part) was not registered, when offsets decrease or run past n_bytes, or when a group has n_reads == 0 or fewer ids than
 * members.  Two things differ from what smr_report_add leaves behind, neither in the file of a part whose references print distinct ids:
 * (1) a group's text is cut into its n_reads entries at tabs, so an id that itself holds a tab (a header with a tab before its first space) is
 * stored as pieces -- adjacent, so the file and the line count are the same, but the entries are not the ids; (2) where several references of
 * the part print the same id (duplicate ids, or several beyond the table, all "*"), their members are appended reference after reference,
 * where smr_report_add has them in read order. */
int smr_report_add_otu(smr_report*, uint32_t index_num, uint32_t part, const uint8_t* bytes, uint64_t n_bytes, const smr_otu_group* groups,
                       uint64_t n_groups, int any_yid_ycov);
/* on != 0: smr_report_add / smr_report_add_pair leave the OTU map alone (smr_report_add_otu brings it); everything else is unaffected */
int smr_report_skip_otu(smr_report*, int on);
/* The streams of smr_fastx_denovo: stream j is appended to the open aligned_denovo file of that index, through gzip under zip_out.
 * SMR_ERR_ARG, and nothing is written, when a stream that is not empty has no open file or the offsets decrease. */
int smr_report_add_denovo(smr_report*, const uint8_t* bytes, const uint64_t off[5]);
/* on != 0: smr_report_add / smr_report_add_pair leave aligned_denovo.* alone (smr_report_add_denovo writes them); everything else is unaffected */
int smr_report_skip_denovo(smr_report*, int on);
/* The gzip members of smr_fastx_split_gz / smr_fastx_denovo_gz: stream k is appended AS IT IS to the open .gz file that smr_report_add_fastx /
 * smr_report_add_denovo would deflate stream k into.  What the file holds from plain calls is closed as a gzip member first and a later plain
 * call begins a new one, so any mix of calls leaves a valid multi-member gzip file that inflates to the streams in call order.  SMR_ERR_ARG,
 * and nothing is appended, when the report was not opened with zip_out, when a stream that is not empty has no open file, or when the offsets
 * decrease.  A report that never sees one of these calls writes the bytes it always wrote. */
int smr_report_add_fastx_gz(smr_report*, const uint8_t* gz, const uint64_t gz_off[9]);
int smr_report_add_denovo_gz(smr_report*, const uint8_t* gz, const uint64_t gz_off[5]);
/* The gzip members of smr_rows_part_gz / smr_pairwise_part_gz for (index_num, part): kept with the rows of that key, behind what the key holds
 * already.  smr_report_close writes the keys in key order as ever and the pieces of a key in call order: plain rows through zlib, members as
 * they are (what zlib holds is closed as a member first).  The SAM header stays plain text and comes first.  Any mix of these calls with
 * smr_report_add / _add_rows / _add_pairwise, over any order of keys, leaves valid multi-member files that inflate to exactly what the plain
 * calls alone would have written.  SMR_ERR_ARG, and nothing is appended: a report not opened with zip_out, a stream that is not empty for a
 * report not opened for it (sam / blast_tabular; blast_pairwise without blast_tabular), decreasing offsets, an (index, part) that was not
 * registered.  A report that never sees one of these calls writes the bytes it always wrote. */
int smr_report_add_rows_gz(smr_report*, uint32_t index_num, uint32_t part, const uint8_t* gz, const uint64_t gz_off[3]);
int smr_report_add_pairwise_gz(smr_report*, uint32_t index_num, uint32_t part, const uint8_t* gz, uint64_t n);
/* *total_otu = lines of otu_map.txt (Readstats::total_otu, for smr_summary), stored when smr_report_close runs: the pointer must live until then */
int smr_report_otu_count(smr_report*, uint64_t* total_otu);
/* One otu_map.txt for a run whose reads went through several report objects (one per device, each fed a contiguous shard of the reads in input
 * order): moves the map entries of `src` behind those of `dst`, per (index, part).  Merged in shard order, every group then lists its reads in
 * (index, part) loop order, then input order, like the reference at -threads 1.  `src` writes no map at its close; `dst` writes the merged one. */
int smr_report_otu_merge(smr_report* dst, smr_report* src);
int smr_report_set_cmdline(smr_report*, const char* cmdline);   /* text after "CL:" in the SAM @PG line (default "libsmr_hip") */
int smr_report_close(smr_report*);      /* writes aligned.blast / aligned.sam, closes the files, frees the object */
const char* smr_report_last_error(const smr_report*);

/* aligned.log: the run summary of Summary::to_string (summary.cpp:102-175), same text for the same numbers.
 * cmdline / pid / timestamp are printed as given (the reference prints its own command line, pid string and ctime()). */
typedef struct {
  const char* ref_file;      /* as given to --ref */
  uint32_t skiplengths[3];
  double lambda, K;          /* Gumbel parameters */
  uint32_t minimal_score;
  uint64_t reads_matched;    /* Readstats::reads_matched_per_db[i] */
} smr_summary_db;
typedef struct {
  const char* cmdline; const char* pid; const char* timestamp;
  uint32_t seed_len; int32_t num_seeds, edges, match, mismatch, gap_open, gap_ext, score_N; int32_t sam_sq; int32_t threads;
  const char* const* reads_files; uint32_t n_reads_files;
  uint64_t total_reads, num_aligned, all_reads_len; uint32_t min_read_len, max_read_len;
  const smr_summary_db* dbs; uint32_t n_dbs;
  /* the two optional Results lines (summary.cpp:139-158) */
  int is_denovo; uint64_t total_denovo;                        /* -de_novo_otu: Readstats::num_denovo */
  int is_otu_map; uint64_t total_id_cov, total_otu;            /* -otu_map: Readstats::n_yid_ycov, lines of otu_map.txt (smr_report_otu_count) */
} smr_summary;
int smr_summary_write(const char* path, const smr_summary*);

/* Readstats persistence: the value Readstats::store_to_db puts into the KVDB after the alignment stage = Readstats::toBstring()
 * (readstats.cpp:133-174, 291-295) and its key = decimal std::hash of the '_'-joined basenames of the read files (readstats.cpp:82-91,
 * util.cpp:216-222).  Both return the size needed; the buffer is filled when it is large enough (the key NUL-terminated). */
size_t smr_readstats_record(uint64_t all_reads_count, uint64_t all_reads_len, uint32_t min_read_len, uint32_t max_read_len, uint64_t num_aligned,
                            uint64_t num_short, const uint64_t* reads_matched_per_db, uint32_t n_db, uint8_t* buf, size_t cap);
size_t smr_readstats_key(const char* const* reads_files, uint32_t n_files, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
