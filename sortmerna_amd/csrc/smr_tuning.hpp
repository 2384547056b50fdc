// smr_tuning.hpp -- the environment switches of libsmr_hip, read in one place (host only; the one file under csrc/ that calls getenv).
// A context reads every switch of its own ONCE, in smr_create (read_tuning), and keeps the result as a const member: setting or deleting a
// variable later changes nothing for that context.  The loaders and builders of smr_index.cpp have no context: their three switches are
// read per call, through the accessors at the end.  None of the switches changes a result.  INTEGRATION.md lists them with the same
// defaults; smr_tuning_text hands out a context's table as it was latched.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>

namespace smr {

// the clamp bounds and defaults that the device headers own (smr_engine.hip fills them in: this header includes none of them)
struct TuningLimits { uint32_t walk_k_max, cand_cap0, cand_cap_max, bloom_words_max, pool_words_min, hot_bin, hot_sub, selfcheck_cases; };

struct Tuning {
  // ---- routes: which kernels run (the parity tests compare every one of them with the oracle)
  int sw_packed = 2;                      // SMR_SW_PACKED: 0 the 32-bit Smith-Waterman kernel only, 1 / 2 the packed 16-bit kernels (smr_sw_pk.hpp; 2 = lane hand-over by wave_ror, measured faster) where they apply
  bool seed_exact = false;                // SMR_SEED_EXACT: the DFS seed kernel for every wave (reference-exact work counters)
  int seed_shared = 1;                    // SMR_SEED_SHARED: one seed sort for the index parts of a batch: 0 off, 1 when the part in hand is not the batch's last, 2 always (tests)
  uint32_t hot_min = 1024;                // SMR_SEED_DEDUP: keys with at least this many tuples in a launch (and four times the average) are searched once per different seed; 0: off   [max(0, .)]
  uint32_t hot_bin = 0;                   // SMR_SEED_HOT_BIN: a coarse key bin is "large" from twice the average and this many tuples (default SEED_HOT_BIN_MIN)   [max(1, .)]
  uint32_t hot_sub = 0;                   // SMR_SEED_HOT_SUB: tuples of a large bin that one block takes (default SEED_HOT_SUB)   [max(1, .)]
  bool seg_inline = true;                 // SMR_SEG_INLINE: 0 = single-hit windows get a pool segment after all (off only for the value 0)
  int handover = 1;                       // SMR_HANDOVER: 0 = k_chain gathers the positions of a marked read itself instead of taking k_cand's record
  int walk_split = 1;                     // SMR_WALK_SPLIT: 0 = k_chain walks every marked read, no candidate walk in rounds (smr_walk.hpp)
  uint32_t walk_rounds = 8;               // SMR_WALK_ROUNDS: rounds per (strand, pass), the last one scores in the kernel   [1..32]
  bool walk_rounds_fixed = false;         //   ... the variable was set: the number does not adapt to what the previous part needed
  uint32_t walk_k = 4;                    // SMR_WALK_K: tasks a read leaves per round, at least (walk_tasks_per_read)   [1..WK_MAX]
  int walk_gather = 1;                    // SMR_WALK_GATHER: 0 = only reads with a record of k_cand go through the rounds (at most 64 positions)
  uint32_t walk_assume = 3;               // SMR_WALK_ASSUME: round 0 predicts "aligns" from this many seeds of the best candidate
  uint32_t walk_prefix = 44;              // SMR_WALK_PREFIX: per cent of a window's columns that a look-ahead task of a read expected to align is scored over (a prefix task, smr_walk.hpp); 0 = off   [0..100]
                                          //   (not in the table below, whose names tests/test_emu_tuning.py pins: smr_walk_prefix_stats hands out what was latched)
  int sw16_f16 = 1;                       // SMR_SW16_F16: 0 = k_sw16 (packed 16-bit integers) scores every task list, 1 = k_sw16h (packed f16, three-operand maxima) where sw_h16_fits holds
                                          //   (not in the table below either: smr_sw16_f16 hands out the mode in use)
  int seed_nbmap = 1;                     // SMR_SEED_NBMAP: the per-key bitmap of the searches that can accept a string (smr_nbmap.hpp): 0 none, 1 where the part is dense enough and the map fits, 2 whatever the density (tests)
  uint32_t nbmap_drop = 1;                //   SMR_SEED_NBMAP_DROP: pattern chars the bitmap leaves out, at least (the policy raises it until the map fits); 1 measured best of 0, 1, 2 on the bench workload (profiles/nbmap_census.log)   [0..SEED_MAXPW]
  uint32_t nbmap_min = 128;               //   SMR_SEED_NBMAP_MIN: strings per present mini-trie from which mode 1 builds (the bench DB has 377, refs8's first member 51, config2's 6; where between 51 and 377 it pays was not measured)
  uint64_t nbmap_bytes = 24ull << 30;     //   SMR_SEED_NBMAP_BYTES: the most a part's bitmap may take (mode 1: and a quarter of the free device memory)
  uint64_t nbmap_alloc_max = ~0ull;       //   SMR_SEED_NBMAP_ALLOC_MAX: test aid, a bitmap larger than this finds no memory (the fall-back to no filter)
                                          //   (none of the five in the table below: smr_seed_nbmap_info hands out what a part got)
  bool begins_x4 = false;                 // SMR_BEGINS_X4 (set): begin cells four per wave (k_begins) instead of sixteen (k_sw16)
  bool pg_host = false;                   // SMR_PG_HOST: the host transform of the pigeonhole layout instead of the device build at upload
  bool trace_global_rows = false;         // SMR_TRACE_GLOBAL_ROWS (set): the wide-band variant of k_trace_wide, rows in global memory
  // ---- capacity test aids: where a pool or table starts (all of them still grow on overflow)
  uint32_t cand_bloom = 128;              // SMR_CAND_BLOOM: Bloom words per read in k_cand   [the next power of two, 64..CAND_BLOOM_WORDS]
  uint32_t ccap = 0;                      // SMR_PG_CAND_CAP: candidate records per wave of k_seed_pg (default PG_CAND_CAP0)   [4..PG_CAND_CAP_MAX]
  uint64_t pool_words = 0;                // SMR_SEED_POOL_WORDS: first size of the seed-hit pool; 0 = from the batch   [base 0; C_NSHARD..0x7FFFFFF0]
  uint64_t cigar_words = 0;               // SMR_CIGAR_POOL_WORDS: first size of a batch's CIGAR pool; 0 = from the batch   [base 10; at least 16]
  uint32_t sw_selfcheck = 0;              // SMR_SW_SELFCHECK: cases of the packed-vs-32-bit self-check in smr_create (default SMR_SW_SELFCHECK_CASES; 0 = skip)
  // ---- diagnostics on stderr (set = on)
  bool verbose = false;                   // SMR_VERBOSE: notices (the table itself, index sizes, capacity growth)
  bool seed_debug = false;                // SMR_SEED_DEBUG: tuples, large bins, hot-key pieces and redo waves of every seed stage (synchronises)
  bool walk_debug = false;                // SMR_WALK_DEBUG: reads listed and tasks left per round (synchronises)
  bool debug_phases = false;              // SMR_DEBUG_PHASES: the phase cycle counters of a -DSMR_CHAIN_PHASES / -DSMR_SEED_PHASES build, in smr_prof_get
};

// name and member of every switch, in the order of the struct (read_tuning fills them, tuning_text prints them)
#define SMR_TUNING_TABLE(X)                                                                                                              \
  X(SMR_SW_PACKED, sw_packed) X(SMR_SEED_EXACT, seed_exact) X(SMR_SEED_SHARED, seed_shared) X(SMR_SEED_DEDUP, hot_min)                   \
  X(SMR_SEED_HOT_BIN, hot_bin) X(SMR_SEED_HOT_SUB, hot_sub) X(SMR_SEG_INLINE, seg_inline) X(SMR_HANDOVER, handover)                     \
  X(SMR_WALK_SPLIT, walk_split) X(SMR_WALK_ROUNDS, walk_rounds) X(SMR_WALK_K, walk_k) X(SMR_WALK_GATHER, walk_gather)                   \
  X(SMR_WALK_ASSUME, walk_assume) X(SMR_BEGINS_X4, begins_x4) X(SMR_PG_HOST, pg_host) X(SMR_TRACE_GLOBAL_ROWS, trace_global_rows)       \
  X(SMR_CAND_BLOOM, cand_bloom) X(SMR_PG_CAND_CAP, ccap) X(SMR_SEED_POOL_WORDS, pool_words) X(SMR_CIGAR_POOL_WORDS, cigar_words)        \
  X(SMR_SW_SELFCHECK, sw_selfcheck) X(SMR_VERBOSE, verbose) X(SMR_SEED_DEBUG, seed_debug) X(SMR_WALK_DEBUG, walk_debug)                 \
  X(SMR_DEBUG_PHASES, debug_phases)

inline Tuning read_tuning(const TuningLimits& L) {
  Tuning t;
  t.hot_bin = L.hot_bin; t.hot_sub = L.hot_sub; t.ccap = L.cand_cap0; t.sw_selfcheck = L.selfcheck_cases;
  const char* e;
  if ((e = getenv("SMR_SW_PACKED"))) t.sw_packed = atoi(e);
  if ((e = getenv("SMR_SEED_EXACT"))) t.seed_exact = atoi(e) != 0;
  if ((e = getenv("SMR_SEED_SHARED"))) t.seed_shared = atoi(e);
  if ((e = getenv("SMR_SEED_DEDUP"))) t.hot_min = (uint32_t)std::max(0, atoi(e));
  if ((e = getenv("SMR_SEED_HOT_BIN"))) t.hot_bin = (uint32_t)std::max(1, atoi(e));
  if ((e = getenv("SMR_SEED_HOT_SUB"))) t.hot_sub = (uint32_t)std::max(1, atoi(e));
  if ((e = getenv("SMR_SEG_INLINE"))) t.seg_inline = atoi(e) != 0;
  if ((e = getenv("SMR_HANDOVER"))) t.handover = atoi(e);
  if ((e = getenv("SMR_WALK_SPLIT"))) t.walk_split = atoi(e);
  if ((e = getenv("SMR_WALK_ROUNDS"))) { t.walk_rounds = (uint32_t)std::max(1, std::min(32, atoi(e))); t.walk_rounds_fixed = true; }
  if ((e = getenv("SMR_WALK_K"))) t.walk_k = (uint32_t)std::max(1, std::min((int)L.walk_k_max, atoi(e)));
  if ((e = getenv("SMR_WALK_GATHER"))) t.walk_gather = atoi(e);
  if ((e = getenv("SMR_WALK_ASSUME"))) t.walk_assume = (uint32_t)atoi(e);
  if ((e = getenv("SMR_WALK_PREFIX"))) t.walk_prefix = (uint32_t)std::max(0, std::min(100, atoi(e)));
  if ((e = getenv("SMR_SW16_F16"))) t.sw16_f16 = atoi(e) != 0 ? 1 : 0;
  if ((e = getenv("SMR_SEED_NBMAP"))) t.seed_nbmap = std::max(0, std::min(2, atoi(e)));
  if ((e = getenv("SMR_SEED_NBMAP_DROP"))) t.nbmap_drop = (uint32_t)std::max(0, std::min(10, atoi(e)));
  if ((e = getenv("SMR_SEED_NBMAP_MIN"))) t.nbmap_min = (uint32_t)std::max(0, atoi(e));
  if ((e = getenv("SMR_SEED_NBMAP_BYTES"))) t.nbmap_bytes = strtoull(e, nullptr, 0);
  if ((e = getenv("SMR_SEED_NBMAP_ALLOC_MAX"))) t.nbmap_alloc_max = strtoull(e, nullptr, 0);
  t.begins_x4 = getenv("SMR_BEGINS_X4") != nullptr;
  if ((e = getenv("SMR_PG_HOST"))) t.pg_host = atoi(e) != 0;
  t.trace_global_rows = getenv("SMR_TRACE_GLOBAL_ROWS") != nullptr;
  if ((e = getenv("SMR_CAND_BLOOM"))) { uint32_t b = 64; while (b < L.bloom_words_max && b < (uint32_t)atoi(e)) b <<= 1; t.cand_bloom = b; }
  if ((e = getenv("SMR_PG_CAND_CAP"))) t.ccap = std::min<uint32_t>(L.cand_cap_max, std::max<uint32_t>(4u, (uint32_t)atoi(e)));
  if ((e = getenv("SMR_SEED_POOL_WORDS"))) t.pool_words = std::min<uint64_t>(std::max<uint64_t>(strtoull(e, nullptr, 0), L.pool_words_min), 0x7FFFFFF0ull);
  if ((e = getenv("SMR_CIGAR_POOL_WORDS"))) t.cigar_words = std::max<uint64_t>(strtoull(e, nullptr, 10), 16);
  if ((e = getenv("SMR_SW_SELFCHECK"))) t.sw_selfcheck = (uint32_t)atoi(e);
  t.verbose = getenv("SMR_VERBOSE") != nullptr;
  t.seed_debug = getenv("SMR_SEED_DEBUG") != nullptr;
  t.walk_debug = getenv("SMR_WALK_DEBUG") != nullptr;
  t.debug_phases = getenv("SMR_DEBUG_PHASES") != nullptr;
  return t;
}

// one NAME=value line per switch, as latched and clamped
inline std::string tuning_text(const Tuning& t) {
  std::string s;
#define SMR_TUNING_LINE(name, member) s += #name "=" + std::to_string(+t.member) + "\n";
  SMR_TUNING_TABLE(SMR_TUNING_LINE)
#undef SMR_TUNING_LINE
  return s;
}

// a notice for SMR_VERBOSE
__attribute__((format(printf, 2, 3))) inline void say(const Tuning& t, const char* fmt, ...) {
  if (!t.verbose) return;
  va_list a;
  va_start(a, fmt);
  fputs("libsmr_hip: ", stderr);
  vfprintf(stderr, fmt, a);
  va_end(a);
}

// ---- no context: read per call
// SMR_HOST_THREADS: caps the host threads of loaders / builders / packers (`cap` = what the machine has)
inline uint32_t tuning_host_threads(uint32_t cap) { const char* e = getenv("SMR_HOST_THREADS"); return e ? std::min<uint32_t>(cap, (uint32_t)std::max(1, atoi(e))) : cap; }
// SMR_LOAD_THREADS: test aid, many loader threads on a small machine (1..256 instead of `dflt`)
inline uint32_t tuning_load_threads(uint32_t dflt) { const char* e = getenv("SMR_LOAD_THREADS"); return e ? std::min<uint32_t>(256, std::max(1, atoi(e))) : dflt; }
// SMR_IB_TIMING (set): stage timings of the index loaders and builders on stderr
inline bool tuning_ib_timing() { return getenv("SMR_IB_TIMING") != nullptr; }

}  // namespace smr
