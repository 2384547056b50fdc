// smr_engine.hip -- device context of libsmr_hip: HBM residency of index parts and the read batch,
// kernel orchestration for one (index, part), capacity regrow/retry, results and profiling.
// Compiled with hipcc --offload-arch=gfx950.  The C ABI is declared in include/smr_hip.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "smr_kernels.hpp"
#include "smr_idcov.hpp"
#include "smr_import.hpp"
#include "smr_export.hpp"
#include "smr_fastx.hpp"
#include "smr_fxsplit.hpp"
#include "smr_rows.hpp"
#include "smr_pairwise.hpp"
#include "smr_mates.hpp"
#include "smr_otu.hpp"
#include "smr_otu_mates.hpp"
#include "smr_gzip.hpp"
#include "smr_gunzip.hpp"
#include "smr_ibuild.hpp"
#include "smr_pgbuild.hpp"
#include "smr_nbmap.hpp"
#include "smr_hostmem.hpp"
#include "smr_devbuf.hpp"
#include "smr_stage.hpp"
#include "smr_score_text.hpp"
#include "smr_tuning.hpp"

using namespace smr;

namespace {

struct DevIndex {
  bool used = false;
  DevBuf<Lookup> lookup; DevBuf<uint32_t> trie, pos_off; DevBuf<uint2> pos_arr;
  DevBuf<uint32_t> pg, root3, lkc;
  // the bitmap of the searches that can accept a string (smr_nbmap.hpp), or one word of ones (nb_words = 0); nb_info = {1 if built, chars dropped,
  // bytes, present mini-tries, their strings, microseconds of the builder kernel} (smr_seed_nbmap_info)
  DevBuf<uint32_t> nbmap; uint32_t nb_words = 0, nb_mask = 0, nb_slabs = 0; uint64_t nb_info[6] = {0, 0, 0, 0, 0, 0};
  DevBuf<uint8_t> ref_seq; DevBuf<uint64_t> ref_off;
  uint32_t n_refs = 0, n_ids = 0, lnwin = 0;
  uint32_t ref_any_n = 1;     // does any reference hold an ambiguous letter (0 only when the upload looked and found none)
  uint64_t trie_words = 0, n_pos = 0, ref_bytes = 0, pg_words = 0;
  // smr_rows_part: the names of the part's references as one text + offsets, uploaded by the first call that sees the slot (rows_part: for which part number)
  DevBuf<uint8_t> rows_names; DevBuf<uint32_t> rows_name_off; int64_t rows_part = -1;
};

struct EvMark { hipEvent_t e; int kind; };        // kind < 0: end of a run of intervals
struct EvPool {                                   // the marks in flight and the events to be used again
  std::vector<EvMark> events; std::vector<hipEvent_t> pool;
  EvPool() = default;
  EvPool(const EvPool&) = delete;
  EvPool& operator=(const EvPool&) = delete;
  ~EvPool() { for (auto& m : events) (void)hipEventDestroy(m.e); for (auto& e : pool) (void)hipEventDestroy(e); }
};

}  // namespace

#define SMR_MAX_BATCHES 16
// kernel families timed apart (one HIP event between them on the engine's stream)
enum { KP_KEYS = 0, KP_SPLIT, KP_BINS, KP_PG0, KP_PG1, KP_FINISH, KP_CAND, KP_CHAIN, KP_BEGINS, KP_TRACE, KP_WALK, KP_SW16, KP_WNEXT, KP_IDCOV, KP_COUNT };
static const char* const KP_NAME[KP_COUNT] = {"k_seed_keys", "k_seed_split", "k_seed_bins", "k_seed_pg<0>", "k_seed_pg<1>", "k_seed_finish", "k_cand", "k_chain", "k_begins", "k_trace",
                                              "k_walk", "k_sw16", "k_wnext", "k_idcov"};

// One resident read batch: packed reads + everything the reference keeps per read in the KVDB (read.cpp:429-539)
// + its Readstats counter block + its CIGAR pool.  Several batches can be resident at once (the host uploads
// batch k+1 while batch k is being aligned); smr_batch_select picks the one the other calls act on.
struct Batch {
  bool used = false;
  uint32_t n = 0, max_len = 0, slots = 1;
  uint32_t min_ge[7] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u};     // the shortest read of at least 8, 10, ... 20 letters (~0: none): what `--edges N%` is smallest for
  uint64_t gen = 0;                        // counts the uploads and state resets of this batch (what a shared seed sort was built for)
  bool min_ge_known = false;               // (computed when a call with is_as_percent asks for it: one pass over the lengths, which the default options never need)
  // (grow-only: a re-upload into the same batch allocates nothing unless it is larger)
  DevBuf<uint32_t> d_words; DevBuf<uint64_t> d_rec_off; DevBuf<uint32_t> d_len;
  DevBuf<RState> d_saved, d_work; DevBuf<RWork> d_rw;
  DevBuf<uint8_t> d_marks;                 // per read: k_chain has to walk it in this (strand, pass) (k_cand)
  DevBuf<AlignRec> d_saved_aln, d_work_aln;
  DevBuf<unsigned long long> d_ctr;
  DevBuf<uint32_t> d_cigar; uint64_t cigar_words = 0;      // (cigar_words: the pool's size as the kernels are told it)
  // the %id / %coverage pass (smr_idcov.hpp): per read {c_yid_ycov, n_yid_ncov, n_nid_ycov, n_denovo} of Read (read.hpp), part of what round-trips
  // through the reference's KVDB; allocated by the first smr_idcov_part of the batch (a run that never asks for the pass pays nothing)
  DevBuf<uint32_t> d_idcov; bool idcov_ran = false;
  std::vector<uint32_t> h_idcov;           // of the reads with alignments, packed like h_state (empty: all zero)
  // host copies of results
  std::vector<RState> h_state; std::vector<AlignRec> h_aln; std::vector<uint32_t> h_cigar;       // of the reads with alignments, packed
  std::vector<uint32_t> h_idx, h_map;                                                            // packed position -> read, read -> packed position (or ~0)
  uint32_t last_num_alignments = 1;
  // SMR_FASTX_KEEP: the FASTA/FASTQ text the batch was parsed from ('\n' behind its fx_n bytes up to a multiple of 16 plus 64) and where every
  // record's header line and first sequence line start in it -- what smr_reads_record_text reads, for smr_fastx_split.  Taken over from the
  // upload's scratch, dropped by any other upload into the batch
  DevBuf<uint8_t> fx_text; DevBuf<unsigned long long> fx_hoff, fx_soff; uint32_t fx_n = 0; bool fx_fastq = false, fx_kept = false;
  unsigned long long redo_seen = 0, win_seen = 0;        // C_SEED_REDO / C_WINDOWS at the end of the previous part (smr_align_part sizes k_seed_pg's candidate pool from the increments)
  bool fetched = false;
};

// (one seed sort for the index parts of a batch: see ensure_shared_sort)
struct SharedSet { DevBuf<SeedTup> srt; DevBuf<uint16_t> wbin; DevBuf<uint32_t> cbase, sn; uint32_t maxwin = 0; bool built = false; };
struct SharedSort {
  SharedSet set[2][3];
  const void* batch = nullptr; uint64_t gen = 0; uint32_t lnwin = 0, skip[3] = {0, 0, 0}, n = 0, max_len = 0;
  uint64_t cap[3] = {0, 0, 0};
  bool usable = false;
  DevBuf<uint32_t> abits;
};
// the owner of the seed-stage scratch; SeedBufs (smr_seed.hpp) is the view of it that the kernels take by value
struct SeedScratch {
  DevBuf<uint32_t> chist, cbase, rows, bcnt, wseg[2], fbits[2], zbits, gflag, emap, sn, redo, hpre, hlist, hh;
  DevBuf<SeedTup> tmp, mid, srt; DevBuf<uint16_t> wbin; DevBuf<uint2> pieces;
};

// scratch of smr_reads_upload_fastx* (smr_fastx.hpp), grow-only; one set per stream the call can run on
struct FxScratch {
  DevBuf<uint8_t> text;
  DevBuf<uint32_t> tot, part_t, part_l, line_start, lrec, lcum, hdr_line, rcum, rlen, rwi;      // part_l: three arrays of one entry per block of lines
  DevBuf<unsigned long long> hoff, soff;
  StageClock<6, 0> clk;                   // (events only: the times of the last call go to smr_ctx::fx_ms under err_m)
};

// scratch and staging of smr_fastx_split (smr_fxsplit.hpp), grow-only
struct FxSplitScratch {
  DevBuf<uint4> rec; DevBuf<unsigned long long> woff, part, tot; DevBuf<uint8_t> hit, out;
  StageClock<6, 4> clk;                   // of the last smr_fastx_split*: measure, scans, copy, D2H
};

// scratch and staging of smr_rows_part (smr_rows.hpp), grow-only; the e-value / bit-score table with the database it was made for
struct RowsScratch {
  DevBuf<uint4> stat, meta; DevBuf<unsigned long long> excl_s, excl_b, part_s, part_b; DevBuf<uint32_t> err; DevBuf<uint8_t> tab, out;
  uint32_t tab_n = 0; double tab_lambda = 0, tab_K = 0; uint64_t tab_ref = 0, tab_read = 0;
  StageClock<7, 4> clk;                   // of the last call: stats, sizes and scans, write, D2H
};

// scratch and staging of smr_otu_part (smr_otu.hpp), grow-only; smr_otu_part_mates (smr_otu_mates.hpp) keeps the per-read part of it once more
// for the mates' batch (pass_m, meta_m, excl_m, part_m)
struct OtuScratch {
  DevBuf<uint8_t> pass, out; DevBuf<uint2> meta; DevBuf<uint4> pairs; DevBuf<uint32_t> key[2], val[2], gstart, err;
  DevBuf<unsigned long long> excl, part, hist, wexcl, wpart, gexcl, gpart; DevBuf<OtuGroup> groups;
  DevBuf<uint8_t> pass_m; DevBuf<uint2> meta_m; DevBuf<unsigned long long> excl_m, part_m;
  StageClock<10, 5> clk;                  // of the last call of either form: classify, size + scans, sort, write, D2H
  StageClock<10, 5> clk_ab[2];            // smr_otu_part_mates: classify and size of the selected batch / of the mates' batch (events 0, 1, 9)
  double compact_ms = 0.0; bool last_mates = false;      // ... its k_otu_mates_pairs; whether the last call was of that form (smr_otu_mates_times)
};

// scratch and staging of the DEFLATE kernels (smr_gzip.hpp), grow-only
struct GzScratch {
  DevBuf<uint8_t> in, slots, out; DevBuf<GzChunk> chunks; DevBuf<GzCode> codes; DevBuf<unsigned long long> slot_off, sizes, cut_tab;
  DevBuf<uint32_t> crc_tab, crc, tok, freq, ntok;
  StageClock<4, 5> clk;                   // of the last call: match, code build, encode, scan + compact, D2H
};

// scratch and staging of the DEFLATE decoder (smr_gunzip.hpp), grow-only; one set per stream smr_reads_upload_fastx* can run on
struct GunzScratch {
  DevBuf<uint32_t> in, n_cand, crc; DevBuf<unsigned long long> cand; DevBuf<GunzTask> tasks; DevBuf<GunzRes> res; DevBuf<GunzUnit> units;
  DevBuf<uint16_t> sym; DevBuf<uint8_t> win, out;
  StageClock<8, 6> clk;                   // of the last call: H2D, find, count, write, window, resolve + CRC (reported through smr_ctx::gunz_ms)
};

struct smr_ctx {
  const Tuning tune;                      // the environment switches as smr_create found them (smr_tuning.hpp)
  explicit smr_ctx(const Tuning& t) : tune(t) {}
  int device = 0;
  DevStream stream, upload_stream;        // upload_stream: smr_reads_upload_batch, H2D of batch k+1 while batch k is aligned on `stream`
  std::string err;                        // last error; written under err_m (smr_reads_upload_batch runs on a second host thread)
  std::mutex err_m, sel_m;                // sel_m: which batch is selected (read by smr_reads_upload_batch)
  int n_cu = 256;
  DevIndex idx[64];
  Batch bt[SMR_MAX_BATCHES];
  Batch* b = &bt[0];
  // pools / scratch (shared by all batches: one batch is aligned at a time)
  DevBuf<uint32_t> d_pool; uint64_t pool_words = 0;
  uint64_t n_pool_grown = 0;              // seed-hit pool regrows (C_ERR_POOL) since smr_create (smr_seed_pool_info)
  uint32_t pool_inline = 0;               // SeedBufs::seg_inline of the last seed-stage launch (smr_seed_pool_info)
  uint32_t hcap = 4;                      // lane-local hit list capacity of k_seed_search; doubles (and the part is redone) on overflow
  int seed_exact = tune.seed_exact;       // 1: k_seed_search for every wave (exact work counters); 0: k_seed_pg (+ redo of the waves whose pool overflowed)
  // Bloom words per read in k_cand (a power of two, 64..512): fewer = more blocks of k_cand per CU, but more reads marked for k_chain by a false
  // collision.  Measured per 2 M-read launch (profiles/r3s18_*): 512 words k_cand 1.07 ms + k_chain 6.01 ms, 256: 0.59 + 6.06, 128: 0.48 + 6.07
  // (16 KB of LDS per block: the 8 blocks per CU that the wave slots allow)
  uint32_t cand_bloom = tune.cand_bloom;
  int seed_shared = tune.seed_shared;     // one seed sort for the index parts of a batch (SharedSort below); 0 for good once its arrays found no room
  DevBuf<uint16_t> d_sw_scr; uint32_t sw_scr_stride = 0;      // scratch rows of the striped Smith-Waterman slow path (smr_sw_striped.hpp), one per block
  int last_seed_slot = -1;                 // index slot of the last smr_seed_scan (smr_seed_hits_fetch translates its ids back)
  SharedSort shared;
  uint64_t n_seed_shared = 0, n_seed_shared_builds = 0;      // smr_prof
  uint32_t ccap = tune.ccap;              // candidate records per wave of k_seed_pg; doubles when more than 1/64 of the waves of a part overflow
  SeedScratch seed; SeedBufs sb = {};     // seed-stage scratch and the kernels' view of it (smr_seed.hpp)
  uint64_t sb_slots = 0; uint32_t sb_nk = 0;
  uint32_t chain_blocks = 0;
  DevBuf<unsigned long long> d_tuples; uint32_t chain_scap = 512;   // (pos, slot, win) tuples; slots of the candidate set S in LDS
  uint32_t keys_need = 0;
  bool chain_ext = false;                                              // a read's candidate set has outgrown the LDS table once: global tables are on
  DevBuf<uint32_t> d_stab; DevBuf<unsigned long long> d_tuples2;       // per block: CH_EXT_CAP-slot table (4 arrays), tuples grouped by member
  size_t chain_lds_attr = 0, begins_lds_attr = 0, split_lds_attr = 0, bins_lds_attr = 0;
  DevBuf<uint32_t> d_fidx; DevBuf<RState> d_fstate; DevBuf<AlignRec> d_faln;       // staging of smr_results_fetch
  DevBuf<uint32_t> d_fidcov;                                                       // ... of the per-read id / coverage counters
  DevBuf<uint8_t> d_xbytes; DevBuf<unsigned long long> d_xoff, d_xpart;            // staging of smr_state_export (d_xpart grows with d_xoff)
  int sw_mode = tune.sw_packed;           // 0 once the packed kernels failed the self-check of smr_create
  // (keys_cap, pairs_cap, hits_cap: per block of k_chain, the layout its kernels are told)
  DevBuf<unsigned long long> d_keys; uint32_t keys_cap = 0;
  DevBuf<unsigned long long> d_pairs; DevBuf<uint32_t> d_lis; uint32_t pairs_cap = 0;
  DevBuf<uint2> d_hits; uint32_t hits_cap = 0;
  DevBuf<uint8_t> d_rdq;
  // k_cand -> k_chain hand-over (smr_chain.hpp): {offset, npos} per read, the records (tune.handover)
  DevBuf<uint2> d_mrec; DevBuf<uint32_t> d_mpool;
  // the candidate walk in rounds (smr_walk.hpp): walk kernel -> Smith-Waterman over a task list -> next list (tune.walk_*)
  DevBuf<uint2> d_wlist[2]; DevBuf<WState> d_wstate[2]; DevBuf<WTask> d_wtask[2]; DevBuf<uint2> d_wres[2];
  DevBuf<uint32_t> d_wtidx, d_wslow; DevBuf<unsigned long long> d_wctr; size_t walk_cap = 0; uint32_t walk_kcap = 0;      // walk_cap x walk_kcap: the layout of d_wtidx
  size_t walk_lds_attr = 0, pg_lds_attr = 0, search_lds_attr = 0;
  int sw16_f16 = tune.sw16_f16;            // k_sw16h (packed f16, smr_walk.hpp) where sw_h16_fits allows it; 0 by SMR_SW16_F16=0, smr_sw16_f16 or a failed self-check of smr_create
  uint64_t sw16h_launches = 0;             // launches of k_sw16h<R> since smr_create, the test seam's included (smr_sw16_f16)
  uint64_t sw16_launches[8] = {};          // k_sw16<13 | 19 | 26 | 32> launched by the walk rounds [0..3] and by the begin-cell stage [4..7] (smr_sw16_launches)
  // rounds per (strand, pass): without SMR_WALK_ROUNDS the number adapts to what the previous part needed (the last round with more than a few
  // reads listed + the closing one: an empty round still costs three launches, ~70 us of stream time; 8 -> 4 rounds = 3 % of the bench step)
  uint32_t walk_need[3] = {0, 0, 0};
  DevBuf<unsigned long long> d_wpstat;     // WPS_N counters of the prefix tasks since smr_prof_reset (smr_walk_prefix_stats)
  bool pfx_live = true; uint32_t pfx_parts_off = 0; unsigned long long pfx_seen[2] = {0, 0};      // adapt_walk_prefix: the mode as the last part's intervals left it; parts since it went off; decided / redone at the last look
  DevBuf<unsigned long long> d_wstat; uint32_t wstat_n = 0; int wstat_pass[8] = {}; uint32_t wstat_rm[8] = {};
  DevBuf<int> d_bound;                                                 // strip-boundary rows of the SW kernels (reads of more than one strip), per block
  DevBuf<uint32_t> d_tasks;                                            // two lists of reads x slots entries
  DevBuf<uint8_t> d_trflags;                                           // direction flags of k_trace_wide (one tile per block)
  DevBuf<int> d_trrows;                                                // its DP rows when the band does not fit LDS
  // profiling
  EvPool ev;
  double kp_ms[KP_COUNT] = {}; uint64_t kp_l[KP_COUNT] = {};       // HIP-event time and launches per kernel family (smr_prof_kernels)
  DevBuf<unsigned long long> d_ctr_snap;    // counters of the selected batch at the start of smr_align_part (restored when an attempt is redone)
  // smr_cand_info (a test seam): what the retry ladder of the last smr_align_part did, and -- once switched on by smr_cand_info_enable -- one byte per
  // read that says which way it went through the candidate stage in the launches of the final attempt (k_cand_route; no other kernel knows of it)
  bool cinfo_on = false; DevBuf<uint8_t> d_croute; uint32_t croute_n = 0;
  uint32_t cinfo_attempts = 0, cinfo_retry[5] = {0, 0, 0, 0, 0};       // attempts; redone because of HITCAP, POOL, PAIRS, REDO, SCAP
  // smr_reads_upload_fastx*: [0] on `stream`, [1] on `upload_stream`; smr_fastx_info / smr_fastx_times of the last call (written under err_m)
  FxScratch fx[2];
  uint64_t fx_info[4] = {0, 0, 0, 0}; double fx_ms[5] = {0, 0, 0, 0, 0};
  FxSplitScratch fxs;
  RowsScratch rows;
  StageClock<7, 4> pair_clk;              // of the last smr_pairwise_part (its device buffers are those of `rows`): guards / statistics, sizes and scans, write, D2H
  // smr_rows_part_mates / smr_pairwise_part_mates (smr_engine_mates.hpp): the scratch of the mates' batch (stat, meta, excl_*, part_*, err, out; the
  // e-value table stays that of `rows`), the interleaved streams, the offsets of smr_interleave_batch, and the clocks of the last call
  RowsScratch rows_m;
  DevBuf<uint8_t> mates_out; DevBuf<unsigned long long> mates_off;
  StageClock<7, 4> mates_clk[2];          // the stages of the selected batch / of the mates' batch
  StageClock<3, 2> mates_zip_clk;         // interleave, D2H
  OtuScratch otu;
  GzScratch gz;
  std::mutex gz_tab_m;                    // the CRC table of `gz` is made at its first use, on either stream
  // the DEFLATE decoder: [0] on `stream`, [1] on `upload_stream`; smr_gunzip_info / _times / _tasks of the last call (written under err_m)
  GunzScratch gunz[2];
  uint64_t gunz_info[8] = {}; double gunz_ms[6] = {}; std::vector<uint64_t> gunz_tasks;
};
struct KpSave { double ms[KP_COUNT]; uint64_t l[KP_COUNT]; };

#define SEED_REDO_CAP 16384u

int dev_fail(smr_ctx* c, const char* call, hipError_t e) {
  std::lock_guard<std::mutex> l_(c->err_m);
  c->err = std::string(call) + ": " + hipGetErrorString(e);
  return SMR_ERR_DEVICE;
}

namespace {

#define HIPCHK(ctx, call)                                          \
  do {                                                             \
    hipError_t e_ = (call);                                        \
    if (e_ != hipSuccess) return dev_fail((ctx), #call, e_);       \
  } while (0)

// every write of the context's error string goes through here (smr_reads_upload_batch runs on a second host thread)
void set_err(smr_ctx* c, const std::string& msg) { std::lock_guard<std::mutex> l_(c->err_m); c->err = msg; }


// a kernel on the engine's stream; the kernel's own parameter types convert the arguments (a DevBuf<T> to T* or const T*)
template <class T> struct arg_of { typedef T type; };
template <class... P> void launch(smr_ctx* c, void (*k)(P...), dim3 grid, dim3 block, size_t lds, typename arg_of<P>::type... a) {
  hipLaunchKernelGGL(k, grid, block, lds, c->stream, a...);
}
// the same on a stream of the caller's choice (smr_reads_upload_fastx_batch works on the upload stream)
template <class... P> void launch_on(hipStream_t st, void (*k)(P...), dim3 grid, dim3 block, size_t lds, typename arg_of<P>::type... a) {
  hipLaunchKernelGGL(k, grid, block, lds, st, a...);
}
// "the dynamic-LDS limit of these kernels is at least `bytes`": set once per high-water mark, and only above what every kernel may use anyway
template <class... F> int raise_lds_limit(smr_ctx* c, size_t& high_water, size_t bytes, size_t free_bytes, F... kernels) {
  if (bytes <= free_bytes || bytes <= high_water) return SMR_OK;
  for (const void* k : {(const void*)kernels...}) HIPCHK(c, hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  high_water = bytes;
  return SMR_OK;
}

const char* scheme_unsupported(int mismatch, int score_N, int gap_open, int gap_ext);
DParams make_dparams(const smr_ctx* c, const DevIndex& di, const smr_params* p) {
  DParams P;
  memset(&P, 0, sizeof P);
  P.lnwin = di.lnwin; P.partialwin = di.lnwin / 2;
  if (p->skiplengths[0] == 0 || p->skiplengths[1] == 0 || p->skiplengths[2] == 0) {   // refstats.cpp:159-166
    P.skip[0] = di.lnwin; P.skip[1] = di.lnwin / 2; P.skip[2] = 3;
  } else { P.skip[0] = p->skiplengths[0]; P.skip[1] = p->skiplengths[1]; P.skip[2] = p->skiplengths[2]; }
  P.num_seeds = p->num_seeds; P.min_lis = p->min_lis; P.edges = p->edges; P.is_as_percent = p->is_as_percent;
  P.match = p->match; P.mismatch = p->mismatch; P.score_N = p->score_N; P.gap_open = p->gap_open; P.gap_ext = p->gap_ext;
  P.minimal_score = p->minimal_score; P.num_alignments = p->num_alignments;
  P.is_best = p->is_best; P.is_full_search = p->is_full_search; P.is_forward = p->is_forward; P.is_reverse = p->is_reverse;
  P.minoccur = p->minoccur; P.index_num = p->index_num; P.part = p->part; P.is_last_index_part = p->is_last_index_part;
  P.slots = c->b->slots;
  // a scheme under which ssw.c's striped kernels leave the affine recurrence: the slow path that reproduces their stripe geometry (smr_sw_striped.hpp)
  P.sw_mode = scheme_unsupported(p->mismatch, p->score_N, p->gap_open, p->gap_ext) ? -1 : c->sw_mode;
  P.sw_scratch = c->d_sw_scr; P.sw_scratch_stride = c->sw_scr_stride;
  return P;
}

// nullptr when the FAST Smith-Waterman kernels here (the affine recurrence H = max(0, diag + s, E, F)) give ssw.c's results under the scheme, else why not
// -- such a scheme goes through the slow path that reproduces ssw.c's stripe geometry (smr_sw_striped.hpp; rounds 1 - 5 refused it).
// (1) The reference's striped kernels store E before the lazy-F loop has raised H (ssw.c:267,496): a gap in one sequence directly after a gap in
// the other is missed when the second crosses a SIMD stripe.  Under 2 * gap_open >= |mismatch| and 2 * gap_ext >= |mismatch| such paths are never
// optimal.  (2) Its 16-bit kernel leaves the lazy-F loop as soon as no lane has F - gap_ext > H - gap_open (ssw.c:496-507); with gap_open <= gap_ext
// that is already true one cell behind a stripe boundary, so a longer gap across a boundary is lost whenever the score needs the 16-bit kernel
// (>= 255 - bias: a 150-nt read's good alignments).  Measured against ssw.c itself on seeded pairs: 2 / -3 / 3 / 3 and 2 / -3 / 2 / 3 differ in
// 1 - 5 % of the high-scoring pairs, every scheme with gap_open > gap_ext in none (tests/test_oracle_golden.py).
const char* scheme_unsupported(int mismatch, int score_N, int gap_open, int gap_ext) {
  const int mm = std::max(-mismatch, -std::min(score_N, 0));
  if (2 * gap_open < mm || 2 * gap_ext < mm) return "scoring scheme outside the supported range (2*gap_open and 2*gap_ext must be >= |mismatch|)";
  // (3) rows and columns beyond the end of a sequence are scored as N by the packed kernels, which is harmless as long as N never adds to a score
  // (found by tools/fuzz_emu.py: with score_N = +1 and ambiguous letters in the reference a reverse pass ran one row past the start of a read)
  if (score_N > 0) return "scoring scheme outside the supported range (score_N must be <= 0: the kernels pad sequences with N)";
  if (gap_open <= gap_ext) return "scoring scheme outside the supported range (gap_open must be greater than gap_ext: the reference's 16-bit kernel ends its lazy-F loop early otherwise, ssw.c:496-507)";
  return nullptr;
}

// sw: the call scores with the Smith-Waterman kernels (the banded traceback alone is exact under every scheme: smr_cigar_batch)
int check_params(smr_ctx* c, const smr_params* p, bool sw = true) {
  if (!p) { set_err(c, "null params"); return SMR_ERR_ARG; }
  if (p->index_num >= 64) { set_err(c, "index_num must be < 64"); return SMR_ERR_ARG; }
  if ((uint64_t)p->minoccur >= 0x3FFFFFFFull) { set_err(c, "minoccur must be < 2^30 - 1"); return SMR_ERR_ARG; }
  if (p->num_seeds < 1 || p->gap_open < 0 || p->gap_ext < 0 || p->match <= 0 || p->mismatch > 0) { set_err(c, "bad scoring/seed options"); return SMR_ERR_ARG; }
  // the reference's scoring matrix is int8_t (ssw_init, ssw.h:88); the SW kernel keeps a row's scores as 4 signed bytes
  if (p->match > 127 || p->mismatch < -127 || p->score_N > 127 || p->score_N < -127 || p->gap_open > 255 || p->gap_ext > 255) { set_err(c, "scores must fit int8 / gaps uint8 like the reference's"); return SMR_ERR_ARG; }
  // --edges: the reference's parser takes 1..10, nucleotides or percent (options.cpp:676); its geometry is not defined outside (0: `tail > edges - 1` is an
  // unsigned compare, alignment.cpp:320,345 -- the whole rest of the reference becomes the window; larger values: more reads whose window length wraps)
  if (sw && (p->edges < 1 || p->edges > 10)) { set_err(c, "edges must be 1..10 (nucleotides or percent), like the reference's --edges"); return SMR_ERR_ARG; }
  if (p->num_alignments > 0 && p->num_alignments > c->b->slots) { set_err(c, "num_alignments exceeds max_alignments_per_read given to smr_reads_upload"); return SMR_ERR_ARG; }
  return SMR_OK;
}

// stored alignments a call cannot work on, as the guards of smr_idcov_part, k_rows_stat and k_otu_classify count them: SMR_OK when all three are 0
int part_refuse_state(smr_ctx* c, const char* who, uint32_t no_cigar, uint32_t bad_ref, uint32_t past) {
  const std::string W = std::string(who) + ": ";
  if (no_cigar) { set_err(c, W + std::to_string(no_cigar) + " alignments of this (index, part) have no CIGAR yet (call smr_traceback first)"); return SMR_ERR_STATE; }
  if (bad_ref) { set_err(c, W + std::to_string(bad_ref) + " alignments with ref_num out of range"); return SMR_ERR_ARG; }
  if (past) { set_err(c, W + std::to_string(past) + " alignments whose CIGAR runs past its read or its reference"); return SMR_ERR_ARG; }
  return SMR_OK;
}

DIndex dindex(const DevIndex& d) {
  DIndex x; x.lookup = d.lookup; x.trie = d.trie; x.pg = d.pg; x.lkc = d.lkc; x.root3 = reinterpret_cast<const uint2*>(d.root3.get()); x.nbmap = d.nbmap; x.nb_words = d.nb_words; x.nb_mask = d.nb_mask; x.pos_off = d.pos_off; x.pos_arr = d.pos_arr; x.ref_seq = d.ref_seq; x.ref_off = d.ref_off;
  x.n_refs = d.n_refs; x.n_ids = d.n_ids; x.lnwin = d.lnwin; x.partialwin = d.lnwin / 2; x.ref_any_n = d.ref_any_n;
  return x;
}
DReads dreads(const Batch& b) { DReads r; r.words = b.d_words; r.rec_off = b.d_rec_off; r.len = b.d_len; r.n = b.n; r.max_len = b.max_len; return r; }
DReads dreads(const smr_ctx* c) { return dreads(*c->b); }

// blocks of k_chain (the one place that says how many): 3 waves per SIMD by registers
constexpr uint32_t CHAIN_WAVES_PER_CU = 12;
uint32_t chain_blocks(smr_ctx* c) {
  if (c->chain_blocks == 0) c->chain_blocks = (uint32_t)c->n_cu * CHAIN_WAVES_PER_CU;
  return c->chain_blocks;
}
// k_chain's scratch per block; the retry ladder of smr_align_part releases an array (and changes its *_cap) to have it made again here
int ensure_chain_scratch(smr_ctx* c) {
  const size_t nb = chain_blocks(c);
  int rc;
  const uint32_t need_keys = std::max(std::max(c->chain_scap, 1024u), c->keys_need);
  if (c->keys_cap < need_keys) { if ((rc = c->d_keys.alloc(c, nb * need_keys))) return rc; c->keys_cap = need_keys; }
  if (c->pairs_cap == 0) c->pairs_cap = 4096;
  if (!c->d_pairs && ((rc = c->d_pairs.alloc(c, nb * c->pairs_cap)) || (rc = c->d_lis.alloc(c, nb * 2 * c->pairs_cap)) || (rc = c->d_tuples.alloc(c, nb * c->pairs_cap)))) return rc;
  if (c->chain_ext) {
    if (!c->d_stab && (rc = c->d_stab.alloc(c, nb * 4 * CH_EXT_CAP))) return rc;
    if (!c->d_tuples2 && (rc = c->d_tuples2.alloc(c, nb * c->pairs_cap))) return rc;
  }
  if (c->hits_cap == 0) c->hits_cap = 4096;
  if (!c->d_hits && (rc = c->d_hits.alloc(c, nb * c->hits_cap))) return rc;
  return SMR_OK;
}

// A mark = one pooled HIP event on the engine's stream.  The time between a mark of kind k >= 0 and the next mark belongs to kernel
// family k; ev_stop ends a run.  (Kernels of one stream run back to back anyway: a mark costs a barrier packet, no bubble.)
void ev_mark(smr_ctx* c, int kind) {
  EvMark m; m.kind = kind;
  if (!c->ev.pool.empty()) { m.e = c->ev.pool.back(); c->ev.pool.pop_back(); }
  else (void)hipEventCreate(&m.e);
  (void)hipEventRecord(m.e, c->stream);
  c->ev.events.push_back(m);
}
void ev_stop(smr_ctx* c) { ev_mark(c, -1); }
// marks a call that failed half-way left behind (an error return between ev_mark and ev_stop): dropped at the start of the next timed call, or
// ev_collect would pair the dangling mark with the first one of an unrelated run and charge the gap to a kernel family
void ev_drop(smr_ctx* c) {
  for (auto& m : c->ev.events) c->ev.pool.push_back(m.e);
  c->ev.events.clear();
}
void ev_collect(smr_ctx* c) {
  for (size_t i = 0; i + 1 < c->ev.events.size(); i++) {
    const int k = c->ev.events[i].kind;
    float ms = 0;
    if (k >= 0 && hipEventElapsedTime(&ms, c->ev.events[i].e, c->ev.events[i + 1].e) == hipSuccess) { c->kp_ms[k] += ms; c->kp_l[k]++; }
  }
  ev_drop(c);
}
KpSave kp_save(const smr_ctx* c) { KpSave k; memcpy(k.ms, c->kp_ms, sizeof k.ms); memcpy(k.l, c->kp_l, sizeof k.l); return k; }
void kp_restore(smr_ctx* c, const KpSave& k) { memcpy(c->kp_ms, k.ms, sizeof k.ms); memcpy(c->kp_l, k.l, sizeof k.l); }

uint32_t num_windows(uint32_t max_len, uint32_t L, uint32_t stride) {
  return max_len >= L ? (max_len - L + stride) / stride : 1;
}

#include "smr_engine_seed.hpp"
#include "smr_engine_chain.hpp"
}  // namespace


// =================================================================================================
// Device index build (kernels in smr_ibuild.hpp)
// =================================================================================================
#include "smr_engine_ibuild.hpp"

#include "smr_engine_swseam.hpp"

// =================================================================================================
extern "C" int smr_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

extern "C" int smr_create(int device, smr_ctx** out, char* err, size_t errcap) {
  if (!out) return SMR_ERR_ARG;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    if (err && errcap) snprintf(err, errcap, "no HIP device available (%s): libsmr_hip has no CPU fallback", e == hipSuccess ? "count=0" : hipGetErrorString(e));
    return SMR_ERR_DEVICE;
  }
  if (device < 0 || device >= ndev) { if (err && errcap) snprintf(err, errcap, "device %d out of range (%d devices)", device, ndev); return SMR_ERR_ARG; }
  // every switch of the context is read here, once; the bounds and defaults that belong to the device headers go in by value
  const TuningLimits lim = {WK_MAX, PG_CAND_CAP0, PG_CAND_CAP_MAX, CAND_BLOOM_WORDS, C_NSHARD, SEED_HOT_BIN_MIN, SEED_HOT_SUB, SMR_SW_SELFCHECK_CASES};
  auto c = new smr_ctx(read_tuning(lim));                 // (deleting it releases whatever the steps below have made)
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreate(&c->stream.s) != hipSuccess || hipStreamCreate(&c->upload_stream.s) != hipSuccess ||
      c->d_ctr_snap.alloc(c, C_TOTAL) != SMR_OK) {
    if (err && errcap) snprintf(err, errcap, "cannot initialise device %d", device);
    delete c; return SMR_ERR_DEVICE;
  }
  say(c->tune, "environment switches of this context:\n%s", tuning_text(c->tune).c_str());
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->n_cu = prop.multiProcessorCount;
  if (c->b->d_ctr.alloc(c, C_TOTAL) != SMR_OK) { if (err && errcap) snprintf(err, errcap, "hipMalloc failed"); delete c; return SMR_ERR_DEVICE; }
  (void)hipMemset(c->b->d_ctr, 0, C_TOTAL * 8);
  c->b->used = true;
  if (c->sw_mode >= 1) {
    // the packed Smith-Waterman kernel must agree with the 32-bit kernel on this device, or it is not used
    const uint32_t cases = c->tune.sw_selfcheck;
    uint64_t bad = 0;
    if (cases > 0 && (smr_sw_selfcheck(c, cases, 20260926u, 700, &bad) != SMR_OK || bad != 0)) {
      fprintf(stderr, "libsmr_hip: packed Smith-Waterman kernel disagrees with the 32-bit kernel on %llu self-check cases; using the 32-bit kernel\n", (unsigned long long)bad);
      c->sw_mode = 0;
    }
  }
  if (c->sw16_f16) {
    // k_sw16h must agree with k_sw16 on this device (end cells, scores, prefix intervals), or the integer kernel does all the work
    uint64_t bad = 0;
    const uint32_t cases = c->tune.sw_selfcheck;
    if (cases > 0 && (sw16h_selfcheck(c, cases, 20261019u, &bad) != SMR_OK || bad != 0)) {
      say(c->tune, "k_sw16h (packed f16) disagrees with k_sw16 on %llu self-check results; using k_sw16\n", (unsigned long long)bad);
      c->sw16_f16 = 0;
    }
    c->sw16h_launches = 0;                 // (the counter is about the work of the context's user)
  }
  *out = c;
  return SMR_OK;
}

extern "C" void smr_destroy(smr_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  delete c;
}

extern "C" int smr_tuning_text(const smr_ctx* c, char* buf, size_t cap) {
  if (!c) return SMR_ERR_ARG;
  const std::string s = tuning_text(c->tune);
  if (buf && cap > s.size()) memcpy(buf, s.c_str(), s.size() + 1);
  return (int)s.size() + 1;
}

extern "C" const char* smr_last_error(const smr_ctx* c) {
  if (!c) return "null context";
  static thread_local std::string copy;                  // the caller's own copy: another host thread may be setting the next error
  { std::lock_guard<std::mutex> l(const_cast<smr_ctx*>(c)->err_m); copy = c->err; }
  return copy.c_str();
}

namespace {
// The pigeonhole layout of the part in slot d (its lookup table and reference-shaped arena are on the device already): smr_pgbuild.hpp
// The position lists as the kernels read them (round 6): a hit's id IS the place of its list -- id' = pos_off[id] + id --, where a header word
// {positions, original id} stands in front of the positions {pos, seq}.  k_cand / k_walk / k_chain went hit -> pos_off[id], pos_off[id + 1] ->
// pos_arr[...]: two random 128-byte lines and two dependent round trips per hit; now the header and (nearly always) the positions share one line.
__global__ void __launch_bounds__(256) k_pos2_build(const uint32_t* __restrict__ pos_off, const uint2* __restrict__ pos_arr, uint32_t n_ids, uint2* __restrict__ pos2) {
  const uint32_t id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= n_ids) return;
  const uint32_t lo = pos_off[id], n = pos_off[id + 1] - lo;
  uint2* o = pos2 + (size_t)lo + id;
  o[0] = make_uint2(n, id);
  for (uint32_t q = 0; q < n; q++) o[1 + q] = pos_arr[lo + q];
}

int build_pigeonhole_device(smr_ctx* c, DevIndex& d, uint32_t nk, uint32_t pw) {
  DevPool pool;
  const uint32_t nb = 2 * nk;
  IB_GET(cnt, uint32_t, nb); IB_GET(eoff, uint32_t, nb); IB_GET(words, smr::u64, nb); IB_GET(woff, smr::u64, nb); IB_GET(derr, uint32_t, 1);
  HIPCHK(c, hipMemsetAsync(derr, 0, 4, c->stream));
  launch(c, smr::k_pgb_sizes, dim3((nb + 255) / 256), dim3(256), 0, (const Lookup*)d.lookup, (const uint32_t*)d.trie, nk, pw, cnt, words);
  smr::u64 W = 0;
  int rc = dev_scan<smr::u64>(c, pool, words, woff, nb, &W); if (rc) return rc;
  if (W / 3 > 0xFFFFFFF0ull || W / 4 > 0xFFFFFFF0ull) { set_err(c, "pigeonhole arena exceeds 2^34 words"); return SMR_ERR_CAPACITY; }
  uint32_t E = 0;
  if ((rc = dev_scan<uint32_t>(c, pool, cnt, eoff, nb, &E))) return rc;
  if ((rc = d.pg.alloc(c, (size_t)W + 4))) return rc;
  if ((rc = d.root3.alloc(c, (size_t)2 * nb))) return rc;
  HIPCHK(c, hipMemsetAsync(d.pg + W, 0, 16, c->stream));                 // one block of slack: a 16-byte read at the last word stays inside
  IB_GET(estr, uint32_t, E); IB_GET(eid, uint32_t, E); IB_GET(eblk, uint32_t, E);
  IB_GET(k0, smr::u64, E); IB_GET(k1, smr::u64, E); IB_GET(v0, uint32_t, E); IB_GET(v1, uint32_t, E);
  launch(c, smr::k_pgb_collect, dim3((nb + 255) / 256), dim3(256), 0, (const Lookup*)d.lookup, (const uint32_t*)d.trie, nk, pw,
                     (const uint32_t*)cnt, (const uint32_t*)eoff, (const smr::u64*)woff, d.root3, d.pg, estr, eid, eblk, derr, (const uint32_t*)d.pos_off);
  uint32_t herr = 0;                                       // (a block k_pgb_collect refused has no entries written: nothing below may run on them)
  HIPCHK(c, hipMemcpyAsync(&herr, derr, 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (herr) { set_err(c, (herr & 1u) ? "a mini-trie is too large for the pigeonhole layout" : "pigeonhole arena exceeds 2^34 words"); return SMR_ERR_CAPACITY; }
  int blockbits = 1; while ((1u << blockbits) < nb) blockbits++;
  const uint32_t gE = (uint32_t)(((smr::u64)E + 255) / 256);
  for (int order = 0; order < 2 && E; order++) {
    const uint32_t kbits = order == 0 ? 2 * (pw + 1) : 2 * (pw - pw / 2);
    smr::u64 *ka = k0, *kb = k1; uint32_t *va = v0, *vb = v1;
    if (order == 0) launch(c, smr::k_pgb_keys<0>, dim3(gE), dim3(256), 0, (const uint32_t*)estr, (const uint32_t*)eblk, (smr::u64)E, pw, kbits, ka, va);
    else launch(c, smr::k_pgb_keys<1>, dim3(gE), dim3(256), 0, (const uint32_t*)estr, (const uint32_t*)eblk, (smr::u64)E, pw, kbits, ka, va);
    if ((rc = dev_radix_sort(c, pool, ka, kb, va, vb, E, 0, (int)kbits + blockbits))) return rc;
    if (order == 0) launch(c, smr::k_pgb_emit<0>, dim3(gE), dim3(256), 0, (const smr::u64*)ka, (const uint32_t*)va, (smr::u64)E, pw, kbits,
                                       (const uint32_t*)estr, (const uint32_t*)eid, (const uint32_t*)eoff, (const uint32_t*)d.root3, d.pg);
    else launch(c, smr::k_pgb_emit<1>, dim3(gE), dim3(256), 0, (const smr::u64*)ka, (const uint32_t*)va, (smr::u64)E, pw, kbits,
                            (const uint32_t*)estr, (const uint32_t*)eid, (const uint32_t*)eoff, (const uint32_t*)d.root3, d.pg);
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  d.pg_words = W;
  return SMR_OK;
}

// The bitmap of slot d's part (smr_nbmap.hpp), by the policy of SMR_SEED_NBMAP: none when the switch is 0, when mode 1 finds the part too sparse for
// it to pay, when no projection of at least NB_MIN_CHARS chars fits the byte budget, or when the device has no room for it -- never an error.
int build_nbmap(smr_ctx* c, DevIndex& d, uint32_t nk, uint32_t pw) {
  int rc;
  d.nb_words = d.nb_mask = d.nb_slabs = 0;
  for (auto& x : d.nb_info) x = 0;
  if ((rc = d.nbmap.alloc(c, 4))) return rc;
  HIPCHK(c, hipMemsetAsync(d.nbmap, 0xFF, 16, c->stream));
  const Tuning& t = c->tune;
  if (t.seed_nbmap == 0) return SMR_OK;
  const uint32_t nb = 2 * nk;
  DevBuf<unsigned long long> cen;
  if ((rc = cen.alloc(c, 2))) return rc;
  HIPCHK(c, hipMemsetAsync(cen, 0, 16, c->stream));
  launch(c, smr::k_nbmap_census, dim3((nb + 255) / 256), dim3(256), 0, (const uint32_t*)d.root3, nb, cen);
  unsigned long long h[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(h, cen, 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  d.nb_info[3] = h[0]; d.nb_info[4] = h[1];
  if (h[0] == 0 || (t.seed_nbmap == 1 && h[1] < (unsigned long long)t.nbmap_min * h[0])) return SMR_OK;
  uint64_t budget = t.nbmap_bytes;
  if (t.seed_nbmap == 1) {
    size_t mem_free = 0, mem_total = 0;
    if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); return SMR_OK; }
    // (a quarter of what is free: the part is uploaded before its batches, whose buffers, seed-hit pool and regrows come out of the rest)
    budget = std::min<uint64_t>(budget, (uint64_t)mem_free / 4);
  }
  uint32_t drop = t.nbmap_drop;
  auto bytes_at = [&](uint32_t s) { return (uint64_t)nb * smr::nb_slab_words(pw, s) * 4; };
  while (drop < pw && pw - drop >= NB_MIN_CHARS && (pw - drop > NB_MAX_CHARS || bytes_at(drop) > budget)) drop++;
  if (drop >= pw || pw - drop < NB_MIN_CHARS) { say(t, "index part: no search bitmap (none of at least %u pattern chars fits %.2f GB)\n", NB_MIN_CHARS, budget * 1e-9); return SMR_OK; }
  const uint64_t bytes = bytes_at(drop);
  DevBuf<uint32_t> map;                                    // (takes the place of the word of ones only once it is built)
  if (bytes > t.nbmap_alloc_max || !map.try_alloc(bytes / 4)) {
    say(t, "index part: no search bitmap (no room for %.2f GB on the device)\n", bytes * 1e-9);
    return SMR_OK;
  }
  const uint32_t words = (uint32_t)smr::nb_slab_words(pw, drop);
  struct Ev { hipEvent_t e = nullptr; ~Ev() { if (e) (void)hipEventDestroy(e); } } e0, e1;
  HIPCHK(c, hipEventCreate(&e0.e)); HIPCHK(c, hipEventCreate(&e1.e));
  HIPCHK(c, hipEventRecord(e0.e, c->stream));
  launch(c, smr::k_nbmap_build, dim3(nb), dim3(256), (size_t)words * 4, (const uint32_t*)d.root3, (const uint32_t*)d.pg, pw, drop, map.get());
  HIPCHK(c, hipEventRecord(e1.e, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipGetLastError());
  float ms = 0;
  (void)hipEventElapsedTime(&ms, e0.e, e1.e);
  d.nbmap = std::move(map);
  d.nb_words = words; d.nb_mask = (1u << (2 * (pw - drop))) - 1u; d.nb_slabs = nb;
  d.nb_info[0] = 1; d.nb_info[1] = drop; d.nb_info[2] = bytes; d.nb_info[5] = (uint64_t)(ms * 1000.0f);
  say(t, "index part: search bitmap %.2f GB (%u of %u pattern chars, %.0f strings per mini-trie), built in %.1f ms\n", bytes * 1e-9, pw - drop, pw, (double)h[1] / (double)h[0], ms);
  return SMR_OK;
}
}  // namespace

extern "C" int smr_index_upload(smr_ctx* c, const smr_index* ix, int slot) {
  if (!c || !ix || slot < 0 || slot >= 64) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if (c->idx[slot].used) smr_index_unload(c, slot);
  DevIndex& d = c->idx[slot];
  d.lnwin = ix->lnwin; d.n_refs = ix->n_refs(); d.n_ids = ix->n_ids(); d.trie_words = ix->trie.size(); d.n_pos = ix->pos_arr.size() / 2; d.ref_bytes = ix->ref_seq.size();
  int rc;
  smr_build_lkc(*const_cast<smr_index*>(ix));              // (cached in the smr_index under its mutex: concurrent uploads of one host index are safe)
  if ((rc = d.lkc.alloc(c, ix->lkc.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(d.lkc, ix->lkc.data(), ix->lkc.size() * 4, hipMemcpyHostToDevice, c->stream));
  if ((rc = d.lookup.alloc(c, ix->lookup.size()))) return rc;
  if ((rc = d.trie.alloc(c, ix->trie.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(d.lookup, ix->lookup.data(), ix->lookup.size() * sizeof(Lookup), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d.trie, ix->trie.data(), ix->trie.size() * 4, hipMemcpyHostToDevice, c->stream));
  // the position lists: pos_off (which the layout build below and the DFS kernel translate ids with) and pos2 = {header, positions} per seed (k_pos2_build)
  if ((uint64_t)ix->pos_arr.size() / 2 + ix->n_ids() >= 0x7FFFFFF0ull) { set_err(c, "index part limit: positions + distinct seeds < 2^31"); return SMR_ERR_CAPACITY; }
  if ((rc = d.pos_off.alloc(c, ix->pos_off.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(d.pos_off, ix->pos_off.data(), ix->pos_off.size() * 4, hipMemcpyHostToDevice, c->stream));
  {
    DevBuf<uint2> raw;                                      // (gone at the end of this block, however it is left)
    if ((rc = raw.alloc(c, ix->pos_arr.size() / 2))) return rc;
    HIPCHK(c, hipMemcpyAsync(raw, ix->pos_arr.data(), ix->pos_arr.size() * 4, hipMemcpyHostToDevice, c->stream));
    if ((rc = d.pos_arr.alloc(c, ix->pos_arr.size() / 2 + (size_t)d.n_ids + 1))) return rc;
    if (d.n_ids) launch(c, k_pos2_build, dim3((d.n_ids + 255u) / 256u), dim3(256), 0, d.pos_off, raw, d.n_ids, d.pos_arr);
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  // The pigeonhole layout of the tries (what k_seed_pg reads) is built on the device from the arena just uploaded (smr_pgbuild.hpp).  An index
  // that already carries the host-built layout (smr_index_selfcheck, SMR_PG_HOST=1) is uploaded as it is.
  bool host_pg = c->tune.pg_host;
  { std::lock_guard<std::mutex> l_(const_cast<smr_index*>(ix)->pg_mutex); host_pg = host_pg || !ix->root3.empty(); }     // (another context may be inside smr_build_pigeonhole on the same host index)
  if (host_pg) {
    std::string why;
    if (!smr_build_pigeonhole(*const_cast<smr_index*>(ix), 0, why)) { set_err(c, why); return SMR_ERR_CAPACITY; }
    if ((rc = d.pg.alloc(c, ix->pg.size()))) return rc;
    if ((rc = d.root3.alloc(c, ix->root3.size()))) return rc;
    HIPCHK(c, hipMemcpyAsync(d.pg, ix->pg.data(), ix->pg.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d.root3, ix->root3.data(), ix->root3.size() * 4, hipMemcpyHostToDevice, c->stream));
    d.pg_words = ix->pg.size() >= 4 ? ix->pg.size() - 4 : 0;
  } else if ((rc = build_pigeonhole_device(c, d, (uint32_t)ix->lookup.size(), ix->lnwin / 2))) return rc;
  say(c->tune, "index part: tries %.2f GB, pigeonhole arena %.2f GB (%s), positions %.2f GB\n", ix->trie.size() * 4e-9, d.pg_words * 4e-9,
      host_pg ? "host-built" : "built on the device", ix->pos_arr.size() * 4e-9);
  if ((rc = d.ref_seq.alloc(c, ix->ref_seq.size() + 64))) return rc;
  if ((rc = d.ref_off.alloc(c, ix->ref_off.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(d.ref_seq, ix->ref_seq.data(), ix->ref_seq.size(), hipMemcpyHostToDevice, c->stream));
  // (after everything else of the part has its memory: the bitmap takes what is left, or is not built)
  if ((rc = build_nbmap(c, d, (uint32_t)ix->lookup.size(), ix->lnwin / 2))) return rc;
  d.ref_any_n = (!ix->ref_seq.empty() && memchr(ix->ref_seq.data(), 4, ix->ref_seq.size())) ? 1u : 0u;      // (k_sw16 asks each window for its ambiguous letters only then)
  HIPCHK(c, hipMemcpyAsync(d.ref_off, ix->ref_off.data(), ix->ref_off.size() * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  d.used = true;
  return SMR_OK;
}

// the device-built pigeonhole layout of slot `slot` against the host transform of the same index (smr_build_pigeonhole): word for word
extern "C" int smr_index_check_device(smr_ctx* c, int slot, smr_index* ix) {
  if (!c || !ix || slot < 0 || slot >= 64 || !c->idx[slot].used) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const DevIndex& d = c->idx[slot];
  std::string why;
  if (!smr_build_pigeonhole(*ix, 0, why)) { set_err(c, why); return SMR_ERR_CAPACITY; }
  if (ix->pg.size() != d.pg_words + 4) { set_err(c, "pigeonhole layout: the device arena has " + std::to_string(d.pg_words) + " words, the host's " + std::to_string(ix->pg.size() - 4)); return SMR_ERR_STATE; }
  std::vector<uint32_t> r3(ix->root3.size()), pg(ix->pg.size());
  HIPCHK(c, hipMemcpy(r3.data(), d.root3, r3.size() * 4, hipMemcpyDeviceToHost));
  HIPCHK(c, hipMemcpy(pg.data(), d.pg, pg.size() * 4, hipMemcpyDeviceToHost));
  for (size_t q = 0; q < r3.size(); q++) if (r3[q] != ix->root3[q]) { set_err(c, "pigeonhole layout: block table differs at word " + std::to_string(q)); return SMR_ERR_STATE; }
  for (size_t q = 0; q < pg.size(); q++) if (pg[q] != ix->pg.data()[q]) { set_err(c, "pigeonhole layout: arena differs at word " + std::to_string(q)); return SMR_ERR_STATE; }
  return SMR_OK;
}

extern "C" int smr_index_unload(smr_ctx* c, int slot) {
  if (!c || slot < 0 || slot >= 64) return SMR_ERR_ARG;
  c->idx[slot] = DevIndex();
  return SMR_OK;
}

extern "C" int smr_batch_select(smr_ctx* c, int batch) {
  if (!c || batch < 0 || batch >= SMR_MAX_BATCHES) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  Batch& B = c->bt[batch];
  if (!B.d_ctr) {
    int rc = B.d_ctr.alloc(c, C_TOTAL); if (rc) return rc;
    HIPCHK(c, hipMemset(B.d_ctr, 0, C_TOTAL * 8));
  }
  B.used = true;
  { std::lock_guard<std::mutex> l(c->sel_m); c->b = &B; }
  return SMR_OK;
}

extern "C" int smr_set_seed_mode(smr_ctx* c, int exact_counters) {
  if (!c) return SMR_ERR_ARG;
  c->seed_exact = exact_counters ? 1 : 0;
  return SMR_OK;
}

namespace {
int reset_batch(smr_ctx* c, Batch& B, hipStream_t st) {
  B.gen++;
  HIPCHK(c, hipMemsetAsync(B.d_saved, 0, (size_t)B.n * sizeof(RState), st));
  HIPCHK(c, hipMemsetAsync(B.d_saved_aln, 0, (size_t)B.n * B.slots * sizeof(AlignRec), st));
  // the Readstats counters, error flags and cursors start over; the profiling work counters (windows .. SW cells, scored-ahead counts and
  // their shards) keep accumulating until smr_prof_reset, like the kernel times do
  HIPCHK(c, hipMemsetAsync(B.d_ctr, 0, (size_t)C_WINDOWS * 8, st));
  HIPCHK(c, hipMemsetAsync(B.d_ctr + C_ERR_HITCAP, 0, (size_t)(C_SW_SPEC - C_ERR_HITCAP) * 8, st));
  HIPCHK(c, hipMemsetAsync(B.d_ctr + C_PCUR, 0, (size_t)C_NSHARD * C_PCUR_STRIDE * 8, st));
  HIPCHK(c, hipMemsetAsync(B.d_ctr + C_IDCOV, 0, 4 * 8, st));
  if (B.d_idcov) HIPCHK(c, hipMemsetAsync(B.d_idcov, 0, std::min(B.d_idcov.cap() / 4, (size_t)B.n) * 16, st));
  B.idcov_ran = false;
  HIPCHK(c, hipStreamSynchronize(st));
  B.fetched = false;
  return SMR_OK;
}
// room in batch B for n reads of `words` packed words and max_aln alignments each, and the batch's fields; the arrays' contents are the caller's
int batch_reserve(smr_ctx* c, Batch& B, size_t words, uint32_t n, uint32_t min_len, uint32_t max_len, uint32_t max_aln, hipStream_t st) {
  int rc;
  if (B.fx_kept) { B.fx_text.release(); B.fx_hoff.release(); B.fx_soff.release(); B.fx_n = 0; B.fx_kept = false; }      // (the text of the reads that are being replaced)
  if (!B.d_ctr) { if ((rc = B.d_ctr.alloc(c, C_TOTAL))) return rc; HIPCHK(c, hipMemsetAsync(B.d_ctr, 0, C_TOTAL * 8, st)); }
  const size_t nw = words + 4, nr = (size_t)n + 1, na = std::max<size_t>((size_t)n * max_aln, 1);     // + slack: window extraction reads 2 words ahead
  if ((rc = B.d_words.reserve(c, nw))) return rc;
  // (the six per-read arrays are reserved for the same number in the same calls: they grow together)
  if ((rc = B.d_rec_off.reserve(c, nr)) || (rc = B.d_len.reserve(c, nr)) || (rc = B.d_saved.reserve(c, nr)) || (rc = B.d_work.reserve(c, nr)) || (rc = B.d_rw.reserve(c, nr)) ||
      (rc = B.d_marks.reserve(c, nr))) return rc;
  if ((rc = B.d_saved_aln.reserve(c, na)) || (rc = B.d_work_aln.reserve(c, na))) return rc;
  B.n = n; B.max_len = max_len; B.slots = max_aln; B.used = true;
  for (int k = 0; k < 7; k++) B.min_ge[k] = ~0u;
  B.min_ge_known = false;
  if (n && min_len >= 100) { for (int k = 0; k < 7; k++) B.min_ge[k] = min_len; B.min_ge_known = true; }      // (1 % of 100 letters is a margin already: nothing to look for)
  return SMR_OK;
}
// the per-read state of a batch whose reads have just been put in place
int batch_fresh_state(smr_ctx* c, Batch& B, hipStream_t st) {
  HIPCHK(c, hipMemsetAsync(B.d_rw, 0, (size_t)B.n * sizeof(RWork), st));
  HIPCHK(c, hipMemsetAsync(B.d_work, 0, (size_t)B.n * sizeof(RState), st));
  B.cigar_words = 0; B.d_cigar.release();
  if (B.d_idcov.cap() < (size_t)B.n * 4) B.d_idcov.release();                     // (the next smr_idcov_part allocates it for this batch size)
  return reset_batch(c, B, st);
}
// the packed reads of r into batch B (+ its per-read state, reset), all work on stream st; touches nothing but B
int upload_into(smr_ctx* c, Batch& B, const smr_reads* r, uint32_t max_aln, hipStream_t st) {
  if (r->view) { set_err(c, "the batch was made with SMR_FASTX_VIEW: its packed words are on the device only"); return SMR_ERR_STATE; }
  if (max_aln == 0) max_aln = 1;
  int rc;
  if ((rc = batch_reserve(c, B, r->words.size(), r->n, r->min_len, r->max_len, max_aln, st))) return rc;
  HIPCHK(c, hipMemcpyAsync(B.d_words, r->words.data(), r->words.size() * 4, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemcpyAsync(B.d_rec_off, r->rec_off.data(), r->rec_off.size() * 8, hipMemcpyHostToDevice, st));
  if (r->n) HIPCHK(c, hipMemcpyAsync(B.d_len, r->len.data(), r->len.size() * 4, hipMemcpyHostToDevice, st));
  return batch_fresh_state(c, B, st);
}
}  // namespace

extern "C" const char* smr_params_refused(const smr_params* p) {
  if (!p) return "null params";
  if (p->edges < 1 || p->edges > 10) return "edges must be 1..10 (nucleotides or percent), like the reference's --edges";
  return nullptr;
}

extern "C" int smr_state_reset(smr_ctx* c) {
  if (!c || !c->b->d_saved) return SMR_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  return reset_batch(c, *c->b, c->stream);
}

extern "C" int smr_reads_upload(smr_ctx* c, const smr_reads* r, uint32_t max_aln) {
  if (!c || !r) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  return upload_into(c, *c->b, r, max_aln, c->stream);
}

// The same into batch `batch`, without selecting it, on the context's UPLOAD stream: may be called from a second host thread while the
// first one is inside smr_align_part / smr_traceback / smr_results_fetch of ANOTHER batch (the two calls share no device buffer: each
// batch owns its reads, per-read state, counters and CIGAR pool; the scratch of the kernels is sized inside smr_align_part).
extern "C" int smr_reads_upload_batch(smr_ctx* c, int batch, const smr_reads* r, uint32_t max_aln) {
  if (!c || !r || batch < 0 || batch >= SMR_MAX_BATCHES) return SMR_ERR_ARG;
  {
    std::lock_guard<std::mutex> l(c->sel_m);
    if (&c->bt[batch] == c->b) { std::lock_guard<std::mutex> l2(c->err_m); c->err = "smr_reads_upload_batch: the batch is the selected one (use smr_reads_upload)"; return SMR_ERR_STATE; }
  }
  HIPCHK(c, hipSetDevice(c->device));
  return upload_into(c, c->bt[batch], r, max_aln, c->upload_stream);
}

namespace {
int ensure_pool(smr_ctx* c) {          // seed-hit pool: scratch shared by all batches, sized for the selected one before its kernels run
  uint64_t want_pool = std::max<uint64_t>((uint64_t)c->b->n * 64 + (1u << 20), 1u << 22);
  if (c->tune.pool_words) want_pool = c->tune.pool_words;     // test aid: start the pool small (regrow) or large (offsets above 2^30)
  if (c->pool_words < want_pool) { int rc = c->d_pool.alloc(c, want_pool); if (rc) return rc; c->pool_words = want_pool; }
  return SMR_OK;
}

int grow_pool(smr_ctx* c) {            // a seed kernel found its shard of the pool full (C_ERR_POOL): twice the words, the attempt is redone
  const uint64_t w = c->pool_words * 2;
  if (w > 0x7FFFFFF0ull) { set_err(c, "seed-hit pool exceeds 8 GiB"); return SMR_ERR_CAPACITY; }
  int rc = c->d_pool.alloc(c, w); if (rc) return rc;
  c->pool_words = w; c->n_pool_grown++;
  return SMR_OK;
}
}  // namespace

__global__ void k_ctr_begin(unsigned long long* __restrict__ ctr, const unsigned long long* __restrict__ snap) {
  for (int k = threadIdx.x; k < C_TOTAL; k += blockDim.x) {
    const bool zero = k == C_NUM_SHORT || (k >= C_ERR_HITCAP && k <= C_ERR_TRACE) || k == C_ERR_SCAP || k == C_ERR_REDO || k == C_POOL_CURSOR || k == C_WORK_NEXT || k >= C_PCUR;
    ctr[k] = zero ? 0ull : snap[k];
  }
}

namespace {
// --edges N% of a read of fewer than 100 / N letters is 0, and 0 is not "no margin" in the reference: `tail > edges - 1` is an unsigned compare
// (alignment.cpp:320,345), so such a read is aligned against the whole rest of its reference sequence.  Not built here (the windows of the
// Smith-Waterman kernels are sized read + 2 x edges): said before anything runs, not as a capacity error of some kernel.
int refuse_percent_edges(smr_ctx* c, const DevIndex& di, const smr_params* p) {
  if (!p->is_as_percent) return SMR_OK;
  Batch& B = *c->b;
  if (!B.min_ge_known) {                                      // the shortest searchable read of the batch, per seed length: from the lengths on the device, once per batch
    std::vector<uint32_t> len(B.n);
    if (B.n) { HIPCHK(c, hipMemcpyAsync(len.data(), B.d_len, (size_t)B.n * 4, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
    for (uint32_t l : len) for (int k = 0; k < 7; k++) if (l >= 8u + 2u * (uint32_t)k && l < B.min_ge[k]) B.min_ge[k] = l;
    B.min_ge_known = true;
  }
  const uint32_t lmin = B.min_ge[(std::min<uint32_t>(std::max<uint32_t>(di.lnwin, 8u), 20u) - 8u) / 2u];
  if (lmin != ~0u && (uint32_t)((p->edges / 100.0) * (double)lmin) == 0) {
    set_err(c, "edges as a percentage: the batch has a searchable read so short that the percentage rounds to 0 letters; the reference then aligns it against the whole rest of the reference sequence (alignment.cpp:320,345), which is not supported -- use an absolute --edges");
    return SMR_ERR_ARG;
  }
  return SMR_OK;
}

// the striped slow path: per block of k_chain / k_begins five arrays of 16 x ceil(len / 8) uint16 (smr_sw_striped.hpp)
int ensure_striped_scratch(smr_ctx* c, DParams& P, const smr_params* p) {
  const uint32_t stride = 5u * 16u * ((c->b->max_len + 7u) / 8u + 1u);
  const size_t need = (size_t)std::max<uint32_t>(chain_blocks(c), (uint32_t)c->n_cu * 8u) * stride;
  if (c->d_sw_scr.cap() < need || c->sw_scr_stride < stride) { int rc = c->d_sw_scr.alloc(c, need); if (rc) return rc; c->sw_scr_stride = stride; }
  P.sw_scratch = c->d_sw_scr; P.sw_scratch_stride = c->sw_scr_stride;
  say(c->tune, "scoring scheme %d/%d/%d (N %d): %s -- Smith-Waterman through the slow path that reproduces ssw.c's stripe geometry\n",
      p->match, p->mismatch, p->gap_open, p->score_N, scheme_unsupported(p->mismatch, p->score_N, p->gap_open, p->gap_ext));
  return SMR_OK;
}

// one attempt at the part: the counters back to the snapshot, then the seed and the candidate stage of every (strand, pass)
int run_attempt(smr_ctx* c, const DevIndex& di, const DParams& P, const smr_params* p, const AlignPlan& plan) {
  Batch& B = *c->b;
  int rc = ensure_chain_scratch(c); if (rc) return rc;
  c->cinfo_attempts++;
  if (c->cinfo_on) {                                          // the route bytes start over with every attempt: they describe the one that is kept
    if ((rc = c->d_croute.reserve(c, B.n))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_croute, 0, (size_t)B.n, c->stream));
    c->croute_n = B.n;
  }
  c->wstat_n = 0;
  const uint32_t tb = 256, nb = (B.n + tb - 1) / tb;
  const int single = (p->is_forward != 0) ^ (p->is_reverse != 0);
  // restore counters (retry) and clear the per-part ones (processor.cpp:230 resets num_short per part)
  launch(c, k_ctr_begin, dim3(1), dim3(256), 0, B.d_ctr, c->d_ctr_snap);
  launch(c, k_begin_part, dim3(nb), dim3(tb), 0, dreads(c), P, B.d_saved, B.d_saved_aln, B.d_work, B.d_work_aln, B.d_rw, B.d_ctr);
  for (int count = 0; count < (single ? 1 : 2); count++) {
    launch(c, k_begin_strand, dim3(nb), dim3(tb), 0, B.n, P, count, B.d_work, B.d_rw);
    HIPCHK(c, hipMemsetAsync(&B.d_ctr[C_PCUR], 0, C_NSHARD * C_PCUR_STRIDE * 8, c->stream));
    for (int pass = 0; pass < 3; pass++) {
      if (pass > 0 && P.skip[pass] == P.skip[pass - 1]) continue;     // equal strides are skipped (paralleltraversal.cpp:269-272)
      if ((rc = launch_seed(c, di, P, pass, !p->is_last_index_part, ((single && p->is_reverse) || count == 1) ? 1 : 0))) return rc;
      if ((rc = launch_chain(c, di, P, plan, pass, single || count == 1))) return rc;
    }
  }
  HIPCHK(c, hipGetLastError());
  return SMR_OK;
}

// The counters h of a finished attempt: what overflowed is enlarged and the attempt has to be redone (retry); what no retry cures is an error.
int judge_attempt(smr_ctx* c, const DParams& P, const std::vector<unsigned long long>& h, bool& retry) {
  int rc;
  retry = false;
  if (h[C_ERR_HITCAP]) { c->cinfo_retry[0]++; if (!grow_hcap(c, P.partialwin)) return SMR_ERR_CAPACITY; retry = true; }
  if (h[C_ERR_POOL]) { c->cinfo_retry[1]++; if ((rc = grow_pool(c))) return rc; retry = true; }
  if (h[C_ERR_PAIRS]) {                                       // (ensure_chain_scratch makes the released arrays again, for the new capacities)
    c->cinfo_retry[2]++;
    c->pairs_cap *= 4; c->hits_cap *= 4; c->d_pairs.release(); c->d_lis.release(); c->d_hits.release(); c->d_tuples.release(); c->d_tuples2.release();
    if (c->pairs_cap > (1u << 22)) { set_err(c, "per-read candidate scratch exceeds capacity"); return SMR_ERR_CAPACITY; }
    retry = true;
  }
  if (h[C_ERR_REDO]) { c->cinfo_retry[3]++; c->seed_exact = 1; retry = true; }     // too many overflowing waves for the redo list: use the DFS kernel throughout
  {
    // k_seed_pg's candidate pool: when more than 1/64 of this part's waves overflowed it (they were searched again by the DFS kernel:
    // right, but slow), the next launches get twice the pool
    Batch& B = *c->b;
    if (h[C_SEED_REDO] < B.redo_seen || h[C_WINDOWS] < B.win_seen) B.redo_seen = B.win_seen = 0;       // counters were reset
    const unsigned long long redo = h[C_SEED_REDO] - B.redo_seen, waves = (h[C_WINDOWS] - B.win_seen) / 32;   // forward + reverse search per window
    B.redo_seen = h[C_SEED_REDO]; B.win_seen = h[C_WINDOWS];
    if (!retry && redo * 64 > waves && c->ccap < PG_CAND_CAP_MAX) {
      c->ccap *= 2;
      say(c->tune, "%llu of ~%llu seed-search waves overflowed their candidate pool: %u records per wave from now on\n", redo, waves, c->ccap);
    }
  }
  if (h[C_ERR_SCAP]) {
    // a read shares seeds with more references than the LDS table of its wave holds (384): from now on such reads build their set in a
    // per-block table in global memory; the candidate keys need room for as many members
    if (c->chain_ext) { set_err(c, "more than 49152 references share seeds with one read (candidate set capacity)"); return SMR_ERR_CAPACITY; }
    c->chain_ext = true; retry = true; c->cinfo_retry[4]++;
    say(c->tune, "a read shares seeds with more references than its wave's LDS table holds: per-block global candidate tables enabled (%.1f GB)\n",
        (double)c->chain_blocks * (4.0 * CH_EXT_CAP * 4 + (double)c->pairs_cap * 8 + (double)CH_EXT_CAP * 8) / 1e9);
    if (c->keys_cap < CH_EXT_CAP) { c->d_keys.release(); c->keys_cap = 0; c->keys_need = CH_EXT_CAP; }
  }
  if (h[C_ERR_SLOTS]) { set_err(c, "a read produced more alignments than max_alignments_per_read (smr_reads_upload)"); return SMR_ERR_CAPACITY; }
  return SMR_OK;
}
}  // namespace

extern "C" int smr_align_part(smr_ctx* c, int slot, const smr_params* p) {
  if (!c || slot < 0 || slot >= 64) return SMR_ERR_ARG;
  if (!c->idx[slot].used || !c->b->d_saved) { set_err(c, "index slot empty or no reads uploaded"); return SMR_ERR_STATE; }
  if (c->b->idcov_ran) { set_err(c, "smr_align_part after smr_idcov_part: the id / coverage pass counts final alignments (denovo_stats runs after align, processor.cpp:368); smr_state_reset or upload first"); return SMR_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  int rc = check_params(c, p); if (rc) return rc;
  const DevIndex& di = c->idx[slot];
  if (di.lnwin < 8 || di.lnwin > 20) { set_err(c, "unsupported seed length"); return SMR_ERR_ARG; }
  DParams P = make_dparams(c, di, p);
  if ((rc = refuse_percent_edges(c, di, p))) return rc;
  const AlignPlan plan = align_plan(c, P);
  if (plan.lds > 150 * 1024) { set_err(c, "reads too long for this build of the SW kernel (LDS)"); return SMR_ERR_CAPACITY; }
  c->b->last_num_alignments = p->num_alignments;
  c->b->fetched = false;
  ev_drop(c);
  if (c->b->n == 0) return SMR_OK;
  if ((rc = ensure_pool(c))) return rc;
  if (plan.striped && (rc = ensure_striped_scratch(c, P, p))) return rc;
  std::vector<unsigned long long> h;
  // the counters as they stand now stay on the device; an attempt that has to be redone starts from them again (one read-back per attempt, none before)
  HIPCHK(c, hipMemcpyAsync(c->d_ctr_snap, c->b->d_ctr, C_TOTAL * 8, hipMemcpyDeviceToDevice, c->stream));
  c->cinfo_attempts = 0;
  for (int q = 0; q < 5; q++) c->cinfo_retry[q] = 0;
  for (int attempt = 0; attempt < 16; attempt++) {            // (the hit-list ladder of the DFS kernel alone has seven steps: grow_hcap)
    const KpSave kp0 = kp_save(c);
    if ((rc = run_attempt(c, di, P, p, plan))) return rc;
    if ((rc = read_ctr(c, h))) return rc;
    ev_collect(c);
    bool retry;
    if ((rc = judge_attempt(c, P, h, retry))) return rc;
    if (retry) { kp_restore(c, kp0); continue; }              // (the timings of a discarded attempt go with it)
    if ((rc = adapt_walk_rounds(c))) return rc;
    if ((rc = adapt_walk_prefix(c))) return rc;
    if ((rc = launch_begins(c, di, P, plan))) return rc;
    // only a clean attempt is committed to the persistent per-read state (kvdb.put, processor.cpp:150-155)
    launch(c, k_commit_part, dim3((c->b->n + 255u) / 256u), dim3(256), 0, c->b->n, P, c->b->d_saved, c->b->d_saved_aln, c->b->d_work, c->b->d_work_aln, c->b->d_rw);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    ev_collect(c);
    return SMR_OK;
  }
  set_err(c, "capacity retries exhausted");
  return SMR_ERR_CAPACITY;
}

#include "smr_engine_trace.hpp"
#include "smr_engine_idcov.hpp"
#include "smr_engine_import.hpp"
#include "smr_engine_export.hpp"
#include "smr_engine_gzip.hpp"
#include "smr_engine_gunzip.hpp"
#include "smr_engine_fastx.hpp"
#include "smr_engine_fxsplit.hpp"
#include "smr_engine_rows.hpp"
#include "smr_engine_pairwise.hpp"
#include "smr_engine_mates.hpp"
#include "smr_engine_otu.hpp"
extern "C" int smr_counters(smr_ctx* c, uint64_t* out, uint32_t n_db) {
  if (!c || !out) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<unsigned long long> h;
  int rc = read_ctr(c, h); if (rc) return rc;
  out[0] = h[C_NUM_ALIGNED]; out[1] = h[C_NUM_SHORT];
  for (uint32_t i = 0; i < n_db && i < 64; i++) out[2 + i] = h[C_PER_DB + i];
  return SMR_OK;
}
extern "C" int smr_counters_device(smr_ctx* c, void** dptr, uint32_t* n_u64) {
  if (!c || !dptr || !n_u64) return SMR_ERR_ARG;
  *dptr = c->b->d_ctr; *n_u64 = C_PER_DB + 64;
  return SMR_OK;
}

__global__ void k_ctr_accumulate(const unsigned long long* __restrict__ ctr, unsigned long long* __restrict__ acc, uint32_t n) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) acc[k] += ctr[k < C_PER_DB + 64 ? k : C_IDCOV + (k - (C_PER_DB + 64))];      // 66 .. 69: n_yid_ycov, n_yid_ncov, n_nid_ycov, num_denovo
}
// acc[k] += the selected batch's counter k, k < n_u64 <= the block smr_counters_device hands out, on the device (a host that aligns its
// shard in chunks keeps ONE device block of sums and all-reduces that over the ranks).  k = 66 .. 69 are the four sums of the id / coverage pass
// (smr_idcov_counters), which live elsewhere in the batch's block: a caller that wants them keeps a block of SMR_COUNTERS_WITH_IDCOV u64.
extern "C" int smr_counters_accumulate(smr_ctx* c, void* d_acc, uint32_t n_u64) {
  if (!c || !d_acc || n_u64 > C_PER_DB + 64 + 4 || !c->b->d_ctr) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  launch(c, k_ctr_accumulate, dim3((n_u64 + 127) / 128), dim3(128), 0, (const unsigned long long*)c->b->d_ctr, (unsigned long long*)d_acc, n_u64);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SMR_OK;
}

// the reads that have alignments, packed: read number, state, alignment slots (order = whatever the atomics hand out)
__global__ void k_results_compact(uint32_t n, uint32_t slots, const RState* __restrict__ saved, const AlignRec* __restrict__ saved_aln,
                                  uint32_t* __restrict__ out_idx, RState* __restrict__ out_state, AlignRec* __restrict__ out_aln, unsigned long long* __restrict__ ctr) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  RState s; s.n_align = 0;
  if (r < n) s = saved[r];
  const uint32_t p = block_append(&ctr[C_FETCH_N], s.n_align != 0);
  if (s.n_align == 0) return;
  out_idx[p] = r; out_state[p] = s;
  for (uint32_t k = 0; k < s.n_align && k < slots; k++) out_aln[(size_t)p * slots + k] = saved_aln[(size_t)r * slots + k];
}

// Only the reads that have alignments cross the bus (a tenth of the batch on the bench workload): compacted on the device, then
// read number -> packed position on the host.
extern "C" int smr_results_fetch(smr_ctx* c) {
  if (!c || !c->b->d_saved) return SMR_ERR_STATE;
  HIPCHK(c, hipSetDevice(c->device));
  Batch& B = *c->b;
  int rc;
  const size_t need_r = std::max<size_t>(B.n, 1), need_a = std::max<size_t>((size_t)B.n * B.slots, 1);
  if ((rc = c->d_fidx.reserve(c, need_r)) || (rc = c->d_fstate.reserve(c, need_r)) || (rc = c->d_faln.reserve(c, need_a))) return rc;
  HIPCHK(c, hipMemsetAsync(&B.d_ctr[C_FETCH_N], 0, 8, c->stream));
  if (B.n) launch(c, k_results_compact, dim3((B.n + 1023) / 1024), dim3(1024), 0, B.n, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln,
                              c->d_fidx, c->d_fstate, c->d_faln, B.d_ctr);
  std::vector<unsigned long long> h;
  rc = read_ctr(c, h); if (rc) return rc;
  const uint64_t cw = std::min<uint64_t>(h[C_CIGAR_CURSOR], B.cigar_words);
  const size_t nhit = (size_t)std::min<unsigned long long>(h[C_FETCH_N], B.n);
  B.h_cigar.resize(cw);
  B.h_idx.resize(nhit); B.h_state.resize(nhit); B.h_aln.resize(nhit * B.slots);
  if (nhit) {
    HIPCHK(c, hipMemcpyAsync(B.h_idx.data(), c->d_fidx, nhit * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(B.h_state.data(), c->d_fstate, nhit * sizeof(RState), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(B.h_aln.data(), c->d_faln, nhit * B.slots * sizeof(AlignRec), hipMemcpyDeviceToHost, c->stream));
  }
  if (cw) HIPCHK(c, hipMemcpyAsync(B.h_cigar.data(), B.d_cigar, cw * 4, hipMemcpyDeviceToHost, c->stream));
  B.h_idcov.clear();
  if (B.d_idcov && nhit) {
    if ((rc = c->d_fidcov.reserve(c, need_r * 4))) return rc;
    B.h_idcov.resize(nhit * 4);
    launch(c, k_idcov_gather, dim3((uint32_t)((nhit + 255) / 256)), dim3(256), 0, (const uint32_t*)c->d_fidx, (const unsigned long long*)&B.d_ctr[C_FETCH_N],
                       (const uint32_t*)B.d_idcov, c->d_fidcov);
    HIPCHK(c, hipMemcpyAsync(B.h_idcov.data(), c->d_fidcov, nhit * 16, hipMemcpyDeviceToHost, c->stream));
  }
  B.h_map.assign(B.n, 0xFFFFFFFFu);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (size_t j = 0; j < nhit; j++) B.h_map[B.h_idx[j]] = (uint32_t)j;
  B.fetched = true;
  return SMR_OK;
}

// Read::toBinString read.cpp:429-462 (+ alignment_struct2::toString, s_align2::toString ssw.hpp:106-140)
static size_t record_of(const Batch& B, uint32_t i, uint8_t* buf, size_t cap);
extern "C" size_t smr_result_record(const smr_ctx* c, uint32_t i, uint8_t* buf, size_t cap) { return c ? record_of(*c->b, i, buf, cap) : 0; }
// the same for batch `batch` whichever batch is selected: reads only the host copy smr_results_fetch made of THAT batch, so a second host
// thread can serialise the records of batch k while the first one aligns batch k+1
extern "C" size_t smr_result_record_batch(const smr_ctx* c, int batch, uint32_t i, uint8_t* buf, size_t cap) {
  return (c && batch >= 0 && batch < SMR_MAX_BATCHES) ? record_of(c->bt[batch], i, buf, cap) : 0;
}
static size_t record_of(const Batch& B, uint32_t i, uint8_t* buf, size_t cap) {
  const Batch* const b_ = &B;
  struct { const Batch* b; } cc{b_}; const auto* c = &cc;          // (the body below reads c->b)
  if (!c->b->fetched || i >= c->b->n) return 0;
  const uint32_t j = c->b->h_map[i];
  if (j == 0xFFFFFFFFu) return 0;
  const RState& s = c->b->h_state[j];
  if (s.n_align == 0) return 0;
  const AlignRec* al = c->b->h_aln.data() + (size_t)j * c->b->slots;
  size_t need = 24 + 3 + 2 + 4 + 4 + 8 + 4 + 4 + 8;
  for (uint32_t k = 0; k < s.n_align; k++) need += 8 + 8 + (size_t)(al[k].has_cigar ? al[k].cigar_len : 0) * 4 + 24 + 6 + 1;
  if (!buf || cap < need) return need;
  uint8_t* p = buf;
  auto put = [&](const void* v, size_t n) { memcpy(p, v, n); p += n; };
  uint8_t z8 = 0;
  // Read::c_yid_ycov, n_yid_ncov, n_nid_ycov, n_denovo: zero until smr_idcov_part has run (the reference: until denovo_stats)
  const uint32_t z4[4] = {0, 0, 0, 0};
  const uint32_t* ic = c->b->h_idcov.size() >= 4 * ((size_t)j + 1) ? c->b->h_idcov.data() + 4 * (size_t)j : z4;
  put(&s.lastIndex, 4); put(&s.lastPart, 4); put(ic, 16);
  put(&s.is_done, 1); put(&s.is_hit, 1); put(&z8, 1);
  put(&s.max_SW_count, 2);
  int32_t na = (int32_t)c->b->last_num_alignments; put(&na, 4);      // Read::init: num_alignments = opts.num_alignments (if > 0)
  put(&s.hit_seeds, 4);
  uint64_t asz = 16;
  for (uint32_t k = 0; k < s.n_align; k++) asz += 8 + 8 + (uint64_t)(al[k].has_cigar ? al[k].cigar_len : 0) * 4 + 24 + 6 + 1;
  put(&asz, 8); put(&s.min_index, 4); put(&s.max_index, 4);
  uint64_t nal = s.n_align; put(&nal, 8);
  for (uint32_t k = 0; k < s.n_align; k++) {
    const AlignRec& a = al[k];
    uint64_t cl = a.has_cigar ? a.cigar_len : 0;
    uint64_t rl = 8 + cl * 4 + 24 + 6 + 1; put(&rl, 8); put(&cl, 8);
    if (cl) put(c->b->h_cigar.data() + a.cigar_off, cl * 4);
    put(&a.ref_num, 4); put(&a.ref_begin1, 4); put(&a.ref_end1, 4); put(&a.read_begin1, 4); put(&a.read_end1, 4); put(&a.readlen, 4);
    put(&a.score1, 2); put(&a.part, 2); put(&a.index_num, 2); put(&a.strand, 1);
  }
  return (size_t)(p - buf);
}
extern "C" int smr_result_is_hit(const smr_ctx* c, uint32_t i) {
  if (!c || !c->b->fetched || i >= c->b->n || c->b->h_map[i] == 0xFFFFFFFFu) return 0;
  return c->b->h_state[c->b->h_map[i]].is_hit;
}

// ---- standalone seed scan (kernel-level parity and the seed-scan roofline bench) ------------------
__global__ void k_force_pass(uint32_t n, DParams P, int pass, const uint32_t* __restrict__ len, RWork* __restrict__ rw) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  RWork w = rw[i];
  w.strand_active = len[i] >= P.lnwin ? 1 : 0; w.search = 1; w.pass_n = (uint8_t)pass; w.win_shift = P.skip[pass];
  for (int q = 0; q < 3; q++) w.blk_cnt[q] = 0;
  w.hit_total = 0; w.valid = w.strand_active;
  rw[i] = w;
}

extern "C" int smr_seed_scan(smr_ctx* c, int slot, const smr_params* p, int strand, int pass, uint64_t* n_hits_out) {
  if (!c || slot < 0 || slot >= 64 || pass < 0 || pass > 2) return SMR_ERR_ARG;
  if (!c->idx[slot].used || !c->b->d_saved) { set_err(c, "index slot empty or no reads uploaded"); return SMR_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  int rc = check_params(c, p); if (rc) return rc;
  const DevIndex& di = c->idx[slot];
  DParams P = make_dparams(c, di, p);
  c->last_seed_slot = slot;
  if ((rc = ensure_pool(c))) return rc;
  ev_drop(c);
  const uint32_t tb = 256, nb = (c->b->n + tb - 1) / tb;
  std::vector<unsigned long long> h;
  for (int attempt = 0; attempt < 16; attempt++) {
    HIPCHK(c, hipMemsetAsync(&c->b->d_ctr[C_ERR_HITCAP], 0, 16, c->stream));          // HITCAP, POOL
    HIPCHK(c, hipMemsetAsync(&c->b->d_ctr[C_PCUR], 0, C_NSHARD * C_PCUR_STRIDE * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(&c->b->d_ctr[C_HIT], 0, 8, c->stream));
    HIPCHK(c, hipMemsetAsync(&c->b->d_ctr[C_SHARDS], 0, C_SHARD_W * C_NSHARD * 8, c->stream));
    // fresh per-part/strand state: forward, or reverse-complement with ambiguous letters complemented (aval 0 -> 3)
    launch(c, k_begin_part, dim3(nb), dim3(tb), 0, dreads(c), P, c->b->d_saved, c->b->d_saved_aln, c->b->d_work, c->b->d_work_aln, c->b->d_rw, c->b->d_ctr);
    DParams Q = P; Q.is_forward = 1; Q.is_reverse = 1;
    launch(c, k_begin_strand, dim3(nb), dim3(tb), 0, c->b->n, Q, strand ? 1 : 0, c->b->d_work, c->b->d_rw);
    launch(c, k_force_pass, dim3(nb), dim3(tb), 0, c->b->n, P, pass, c->b->d_len, c->b->d_rw);
    if ((rc = launch_seed(c, di, P, pass))) return rc;
    if ((rc = read_ctr(c, h))) return rc;
    ev_collect(c);
    bool retry = false;
    if (h[C_ERR_HITCAP]) { if (!grow_hcap(c, P.partialwin)) return SMR_ERR_CAPACITY; retry = true; }
    if (h[C_ERR_POOL]) { if ((rc = grow_pool(c))) return rc; retry = true; }
    if (!retry) { if (n_hits_out) *n_hits_out = h[C_HIT]; return SMR_OK; }
  }
  set_err(c, "capacity retries exhausted");
  return SMR_ERR_CAPACITY;
}

// Test seam (the roofline numerator's audit, tests/test_gpu_parity.py): the sorted tuples of the LAST seed-stage launch of this context -- what
// k_seed_pg searched -- and what it takes to decode them: meta = {tuples, forward tuples, coarse bins nc, fine bits fb, char bits cb, nkh,
// candidate records per wave}, cbase[nc + 1].
extern "C" int smr_seed_tuples_fetch(smr_ctx* c, uint64_t* tuples, uint64_t cap_tuples, uint32_t* cbase, uint32_t cap_cbase, uint32_t meta[8]) {
  if (!c || !meta) return SMR_ERR_ARG;
  if (!c->sb.srt || !c->sb.sn) { set_err(c, "no seed stage has run"); return SMR_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  uint32_t sn[SN_COUNT];
  HIPCHK(c, hipMemcpy(sn, c->sb.sn, sizeof sn, hipMemcpyDeviceToHost));
  const uint32_t nt = (uint32_t)std::min<uint64_t>(sn[SN_TUPLES], 2 * c->sb_slots);      // (cap_tuples is a per-launch field of launch_seed's copy; the arrays hold 2 x sb_slots)
  meta[0] = nt; meta[1] = std::min(sn[SN_FWD], nt); meta[2] = c->sb.nc; meta[3] = c->sb.fb; meta[4] = c->sb.cb; meta[5] = c->sb.nkh; meta[6] = c->ccap; meta[7] = sn[SN_REDO];
  if (tuples) { if (cap_tuples < nt) return SMR_ERR_CAPACITY; if (nt) HIPCHK(c, hipMemcpy(tuples, c->sb.srt, (size_t)nt * sizeof(SeedTup), hipMemcpyDeviceToHost)); }
  if (cbase) { if (cap_cbase < c->sb.nc + 1u) return SMR_ERR_CAPACITY; HIPCHK(c, hipMemcpy(cbase, c->sb.cbase, (size_t)(c->sb.nc + 1u) * 4, hipMemcpyDeviceToHost)); }
  return SMR_OK;
}

// Test seam (tests/test_gpu_parity.py, the seed-hit pool at its limits): info = {pool words, regrows since smr_create, one past the highest pool
// word handed out, 1 if the last seed-stage launch inlined one-hit windows}.  The third is max(shard * region + cursor) over the shards with a
// non-zero cursor of the selected batch: what the last attempt's last strand handed out (the cursors restart with each strand).
extern "C" int smr_seed_pool_info(smr_ctx* c, uint64_t info[4]) {
  if (!c || !info) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<unsigned long long> cur(C_NSHARD * C_PCUR_STRIDE, 0ull);
  if (c->b->d_ctr) {
    HIPCHK(c, hipMemcpyAsync(cur.data(), &c->b->d_ctr[C_PCUR], cur.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  const uint64_t region = std::min<uint64_t>(c->pool_words, 0x7FFFFFF0ull) / C_NSHARD;
  uint64_t hi = 0;
  for (int s = 0; s < C_NSHARD; s++) if (cur[s * C_PCUR_STRIDE]) hi = std::max<uint64_t>(hi, s * region + cur[s * C_PCUR_STRIDE]);
  info[0] = c->pool_words; info[1] = c->n_pool_grown; info[2] = hi; info[3] = c->pool_inline;
  return SMR_OK;
}

// Test seams of the search bitmap (smr_nbmap.hpp).  smr_seed_nbmap_info: info = {1 if slot's part has a bitmap, pattern chars it leaves out, its bytes,
// present mini-tries of the part, their strings, microseconds of the builder kernel, then of the SELECTED batch's counters: searches k_seed_pg
// probed, of which their bit was set, of which accepted no string}.  smr_seed_nbmap_fetch: the slabs [first, first + n) of the part (slab 2 * key +
// direction; words_per_slab as info says: 4^(pw - dropped) / 32) into out.
extern "C" int smr_seed_nbmap_info(smr_ctx* c, int slot, uint64_t info[9]) {
  if (!c || !info || slot < 0 || slot >= 64) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const DevIndex& d = c->idx[slot];
  for (int q = 0; q < 6; q++) info[q] = d.used ? d.nb_info[q] : 0;       // (an empty slot: zeros, the counters below all the same)
  std::vector<unsigned long long> h(C_TOTAL, 0ull);
  if (c->b->d_ctr) { int rc = read_ctr(c, h); if (rc) return rc; }        // (the census is sharded like the work counters: folded on the host)
  info[6] = h[C_NB_PROBED]; info[7] = h[C_NB_PASSED]; info[8] = h[C_NB_EMPTY];
  return SMR_OK;
}
extern "C" int smr_seed_nbmap_fetch(smr_ctx* c, int slot, uint64_t first, uint64_t n, uint32_t* out, uint64_t cap_words) {
  if (!c || !out || slot < 0 || slot >= 64 || !c->idx[slot].used) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  const DevIndex& d = c->idx[slot];
  if (!d.nb_words) { set_err(c, "smr_seed_nbmap_fetch: the part has no bitmap"); return SMR_ERR_STATE; }
  if (first > d.nb_slabs || n > d.nb_slabs - first) return SMR_ERR_ARG;
  if (cap_words < n * d.nb_words) return SMR_ERR_CAPACITY;
  if (n) HIPCHK(c, hipMemcpy(out, d.nbmap + first * d.nb_words, n * d.nb_words * 4, hipMemcpyDeviceToHost));
  return SMR_OK;
}

// Test seam (tests/test_gpu_cand_limits.py, the candidate stage at its path boundaries).  smr_cand_info_enable switches the per-read route bytes
// on or off for the calls that follow; the counts of smr_cand_info are kept either way (host integers).
//   info = {attempts of the last smr_align_part, of which redone because of HITCAP, POOL, PAIRS, REDO, SCAP (five words),
//           chain_ext, chain_scap, keys_cap, pairs_cap, hits_cap as they stand now, 1 if the route bytes are on, reads the route bytes cover}
//   smr_cand_routes: the byte of every read, OR-ed over the (strand, pass) launches of the last attempt of the last smr_align_part --
//           SMR_ROUTE_RECORD | SMR_ROUTE_GATHER (listed for k_walk with / without a record of k_cand), SMR_ROUTE_CHAIN (k_chain<false>), SMR_ROUTE_EXT (k_chain<true>)
extern "C" int smr_cand_info_enable(smr_ctx* c, int on) {
  if (!c) return SMR_ERR_ARG;
  c->cinfo_on = on != 0;
  if (!c->cinfo_on) c->croute_n = 0;
  return SMR_OK;
}
extern "C" int smr_cand_info(smr_ctx* c, uint64_t info[13]) {
  if (!c || !info) return SMR_ERR_ARG;
  info[0] = c->cinfo_attempts;
  for (int q = 0; q < 5; q++) info[1 + q] = c->cinfo_retry[q];
  info[6] = c->chain_ext ? 1 : 0; info[7] = c->chain_scap; info[8] = c->keys_cap; info[9] = c->pairs_cap; info[10] = c->hits_cap;
  info[11] = c->cinfo_on ? 1 : 0; info[12] = c->croute_n;
  return SMR_OK;
}
extern "C" int smr_cand_routes(smr_ctx* c, uint8_t* out, uint32_t n) {
  if (!c || !out) return SMR_ERR_ARG;
  if (!c->cinfo_on || !c->d_croute || n != c->croute_n) { set_err(c, "smr_cand_routes: no route bytes for that many reads (smr_cand_info_enable before smr_align_part)"); return SMR_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  if (n) { HIPCHK(c, hipMemcpyAsync(out, c->d_croute, (size_t)n, hipMemcpyDeviceToHost, c->stream)); HIPCHK(c, hipStreamSynchronize(c->stream)); }
  return SMR_OK;
}

extern "C" int smr_seed_hits_fetch(smr_ctx* c, uint32_t* triples, uint64_t cap_triples, uint64_t* n_out) {
  if (!c || !n_out) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<unsigned long long> h;
  int rc = read_ctr(c, h); if (rc) return rc;
  uint64_t words = h[C_POOL_CURSOR] ? std::min<uint64_t>(c->pool_words, 0x7FFFFFF0ull) : 0;   // sharded pool: fetch all regions
  std::vector<uint32_t> pool(words);
  std::vector<RWork> rw(c->b->n);
  if (words) HIPCHK(c, hipMemcpy(pool.data(), c->d_pool, words * 4, hipMemcpyDeviceToHost));
  if (c->b->n) HIPCHK(c, hipMemcpy(rw.data(), c->b->d_rw, (size_t)c->b->n * sizeof(RWork), hipMemcpyDeviceToHost));
  // (the device's ids are places in its position array, id' = pos_off[id] + id: back to the index's ids for the caller)
  std::vector<uint32_t> po;
  if (c->last_seed_slot >= 0 && c->idx[c->last_seed_slot].used) {
    const DevIndex& di = c->idx[c->last_seed_slot];
    po.resize((size_t)di.n_ids + 1);
    HIPCHK(c, hipMemcpy(po.data(), di.pos_off, po.size() * 4, hipMemcpyDeviceToHost));
  }
  auto orig = [&](uint32_t idp) -> uint32_t {
    if (po.size() < 2) return idp;
    size_t lo = 0, hi = po.size() - 1;                      // the last id with pos_off[id] + id <= idp
    while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if ((uint64_t)po[mid] + mid <= idp) lo = mid; else hi = mid; }
    return (uint32_t)lo;
  };
  uint64_t o = 0;
  for (uint32_t r = 0; r < c->b->n; r++) {
    for (int pp = 0; pp < 3; pp++) {
      const uint32_t cnt = rw[r].blk_cnt[pp], bo = rw[r].blk_off[pp];
      for (uint32_t q = 0; q < cnt && (uint64_t)bo + 2 * q + 1 < words; q++) {
        if (triples && o < cap_triples) { triples[3 * o] = r; triples[3 * o + 1] = orig(pool[bo + 2 * q]); triples[3 * o + 2] = pool[bo + 2 * q + 1]; }
        o++;
      }
    }
  }
  *n_out = o;
  return SMR_OK;
}

extern "C" int smr_prof_reset(smr_ctx* c) {
  if (!c) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  for (int k = 0; k < KP_COUNT; k++) { c->kp_ms[k] = 0; c->kp_l[k] = 0; }
  c->n_seed_shared = c->n_seed_shared_builds = 0;
  if (c->d_wpstat) HIPCHK(c, hipMemsetAsync(c->d_wpstat, 0, WPS_N * 8, c->stream));
  for (int k = 0; k < SMR_MAX_BATCHES; k++)
    if (c->bt[k].d_ctr) {
      HIPCHK(c, hipMemsetAsync(&c->bt[k].d_ctr[C_WINDOWS], 0, 9 * 8, c->stream));
      HIPCHK(c, hipMemsetAsync(&c->bt[k].d_ctr[C_SW_SPEC], 0, 3 * 8, c->stream));
      HIPCHK(c, hipMemsetAsync(&c->bt[k].d_ctr[C_TUP_F], 0, C_SHARD_NX * 8, c->stream));
      HIPCHK(c, hipMemsetAsync(&c->bt[k].d_ctr[C_SHARDS], 0, C_SHARD_W * C_NSHARD * 8, c->stream));
    }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SMR_OK;
}
extern "C" int smr_prof_get(smr_ctx* c, smr_prof* o) {
  if (!c || !o) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<unsigned long long> h(C_TOTAL, 0), t(C_TOTAL);
  for (int k = 0; k < SMR_MAX_BATCHES; k++) {
    if (!c->bt[k].d_ctr) continue;
    HIPCHK(c, hipMemcpyAsync(t.data(), c->bt[k].d_ctr, C_TOTAL * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->tune.debug_phases) {
      unsigned long long ph[7] = {0, 0, 0, 0, 0, 0, 0};
      for (int s2 = 0; s2 < C_NSHARD; s2++) for (int q = 0; q < 7; q++) ph[q] += t[C_SHARDS + C_SHARD_W * s2 + C_SHARD_PH + q];
      fprintf(stderr, "[smr] phase cycles (batch %d): %llu %llu %llu %llu %llu %llu %llu  (-DSMR_CHAIN_PHASES: claim, gather+prefix, walk1, walk2+cands, pairs+sort, "
              "window/lis/book, sw; -DSMR_SEED_PHASES (k_seed_pg): setup, directory ranges, entries, -, candidate selection, output, -)\n", k, ph[0], ph[1], ph[2], ph[3], ph[4], ph[5], ph[6]);
    }
    fold_shards(t);
    for (int q = 0; q < C_COUNT; q++) h[q] += t[q];
  }
  o->seed_ms = c->kp_ms[KP_KEYS] + c->kp_ms[KP_SPLIT] + c->kp_ms[KP_BINS] + c->kp_ms[KP_PG0] + c->kp_ms[KP_PG1] + c->kp_ms[KP_FINISH]; o->seed_launches = c->kp_l[KP_KEYS];
  o->chain_ms = c->kp_ms[KP_CAND] + c->kp_ms[KP_CHAIN] + c->kp_ms[KP_BEGINS] + c->kp_ms[KP_WALK] + c->kp_ms[KP_SW16] + c->kp_ms[KP_WNEXT]; o->chain_launches = c->kp_l[KP_CAND] + c->kp_l[KP_BEGINS];
  o->trace_ms = c->kp_ms[KP_TRACE]; o->trace_launches = c->kp_l[KP_TRACE];
  o->n_windows = h[C_WINDOWS]; o->n_lookup = h[C_LOOKUP]; o->n_node = h[C_NODE]; o->n_entry = h[C_ENTRY]; o->n_hit = h[C_HIT]; o->n_read_bytes = h[C_READ_BYTES];
  o->n_sw_fwd = h[C_SW_FWD]; o->n_sw_rev = h[C_SW_REV]; o->n_sw_cells = h[C_SW_CELLS];
  o->n_sw_spec = h[C_SW_SPEC]; o->n_sw_spec_used = h[C_SW_SPEC_USED]; o->n_seed_redo = h[C_SEED_REDO]; o->hit_list_cap = c->hcap;
  o->n_seed_shared = c->n_seed_shared; o->n_seed_shared_builds = c->n_seed_shared_builds;
  return SMR_OK;
}

// Per kernel family: HIP-event time, launches and the algorithmic HBM bytes the kernels counted for themselves (0: not counted)
extern "C" int smr_prof_kernels(smr_ctx* c, smr_kprof* out, uint32_t cap, uint32_t* n_out) {
  if (!c || !out || !n_out) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<unsigned long long> h(C_TOTAL, 0), t(C_TOTAL);
  for (int k = 0; k < SMR_MAX_BATCHES; k++) {
    if (!c->bt[k].d_ctr) continue;
    HIPCHK(c, hipMemcpyAsync(t.data(), c->bt[k].d_ctr, C_TOTAL * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fold_shards(t);
    for (int q = 0; q < C_COUNT; q++) h[q] += t[q];
  }
  const unsigned long long T = h[C_TUP_ALL];
  unsigned long long bytes[KP_COUNT] = {};
  bytes[KP_KEYS] = h[C_B_KEYS] + sizeof(SeedTup) * T;                 // its inputs (counted by the kernel) + every tuple written once
  bytes[KP_SPLIT] = bytes[KP_BINS] = 2 * sizeof(SeedTup) * T;         // each of the two sort passes reads and writes every tuple once
  bytes[KP_PG0] = h[C_B_PG0]; bytes[KP_PG1] = h[C_B_PG1]; bytes[KP_FINISH] = h[C_B_FIN];
  uint32_t n = 0;
  for (int k = 0; k < KP_COUNT && n < cap; k++, n++) {
    memset(&out[n], 0, sizeof out[n]);
    snprintf(out[n].name, sizeof out[n].name, "%s", KP_NAME[k]);
    out[n].ms = c->kp_ms[k]; out[n].launches = c->kp_l[k]; out[n].bytes = bytes[k];
  }
  *n_out = n;
  return SMR_OK;
}
