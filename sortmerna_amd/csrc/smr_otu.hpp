// smr_otu.hpp -- the members of otu_map.txt for the stored alignments of one (index, part), found, grouped and written on the device from what is
// in HBM after smr_idcov_part: the per-read counters, AlignRec and the CIGAR pool, the packed letters, the part's reference letters and the
// kept FASTX text (SMR_FASTX_KEEP).  The definition of every byte is add_otu of smr_report.cpp (the reference: fill_otu_map2,
// otumap.cpp:131-198): a read with c_yid_ycov > 0 has every alignment of the key classified AGAIN -- over the FORWARD letters whatever the
// strand (smr_idcov.hpp), with the rounding written `* 0.001` where the pass divides by 1000.0 -- and joins the group of the reference of
// every alignment that passes both thresholds.
//
//   k_otu_classify  16 lanes per alignment slot, four slots per wave, for CIGARs of up to IDCOV_FEW_OPS operations (idcov_run); a longer CIGAR
//                   is then walked by the whole wave, 64 operations at a time (k_idcov_many's way).  Leaves a pass bit per slot and counts
//                   what the host writer would refuse (err[]: the only atomics of the family).  Changes no stored state.
//   k_otu_size      a thread per read: where its id lies in the text, how many of its slots passed; summed inside the block.
//   k_otu_pairs     a thread per read puts its {ref_num, read, id offset, id length} at the place the sums give: read order, then slot order.
//   k_otu_hist /    a STABLE least-significant-digit radix sort of the pairs by ref_num, 8 bits a pass, as many passes as n_refs needs.  A
//   k_otu_move      wave owns OTU_UNIT consecutive items and takes them 64 at a time; the lanes that hold the same digit find each other
//                   with nine ballots, which gives each its rank among them and their number without any atomic; the lowest lane of a digit
//                   keeps the wave's count of it in LDS.  k_otu_hist leaves the counts per (digit, wave), k_export_scan turns them into
//                   their exclusive sums over digits x waves, k_otu_move walks the same items again, stages them in LDS in digit order and writes the
//                   stage out in order, the items of a digit to consecutive words.  One hot
//                   reference costs what an even spread costs: the counter of a digit is touched once per 64 items, by one lane, in LDS.
//   k_otu_wsize     over the sorted pairs: the bytes of each (id + a tab, the last of a group without it) and the group starts, summed.
//   k_otu_write     a wave takes 64 sorted pairs, a contiguous byte range, and puts them together in an LDS window that starts on an output
//                   dword (RowsWave / exp_flush of smr_rows.hpp: whole dwords coalesced, the range's first and last dword as bytes).
//   k_otu_groups /  the table of groups: reference, first byte, number of members.
//   k_otu_gcount
#pragma once

namespace smr {

#define OTU_UNIT 1024u          // items per wave of the sort
#define OTU_BLOCK 256u          // threads per block of the sizing kernels
enum { OTU_E_NOCIG = 1, OTU_E_PAST, OTU_E_BADREF, OTU_E_ANY, OTU_E_COUNT };      // OTU_E_ANY: not an error, "a read of the batch has c_yid_ycov > 0"

struct OtuGroup { uint32_t ref_num, n_reads; unsigned long long off; };           // smr_otu_group of smr_hip.h

// the decision of fill_otu_map2 (otumap.cpp:166-175).  As in idcov_class the product and the sum stay two operations; the rounded value is
// scaled back with `* 0.001`, which is not always the double that `/ 1000.0` gives (9 * 0.001 > 9 / 1000.0).
__device__ __forceinline__ bool otu_pass(uint32_t n_miss, uint32_t n_gap, uint32_t n_match, int32_t read_begin1, int32_t read_end1, uint32_t readlen,
                                         double min_id, double min_cov) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const uint32_t n_tot = n_miss + n_gap + n_match;
  const int32_t span = read_end1 - read_begin1 + 1;
  const double id = (double)n_match / (double)n_tot;
  const double cov = (double)(span < 0 ? -span : span) / (double)readlen;
  const double id1000 = id * 1000.0, cov1000 = cov * 1000.0;
  const double idr = floor(id1000 + 0.5) * 0.001;
  const double covr = floor(cov1000 + 0.5) * 0.001;
  return idr >= min_id && covr >= min_cov;             // (no columns: 0 / 0, a NaN, passes nothing -- as on the host)
}

// pass[i] = 1 for every alignment slot i of a read with c_yid_ycov > 0 that holds an alignment of (index_num, part) passing both thresholds
__global__ void __launch_bounds__(256) k_otu_classify(DReads rd, DIndex ix, uint32_t slots, const RState* __restrict__ saved, const AlignRec* __restrict__ aln,
                                                      const uint32_t* __restrict__ cigar, unsigned long long pool_words, const uint32_t* __restrict__ idcov,
                                                      uint32_t index_num, uint32_t part, double min_id, double min_cov,
                                                      uint8_t* __restrict__ pass, uint32_t* __restrict__ err) {
  const uint32_t lane = (uint32_t)lane_id(), g = lane >> 4, gl = lane & 15u;
  const unsigned long long total = (unsigned long long)rd.n * slots, n_waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
  for (unsigned long long base = ((unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 4ull; base < total; base += n_waves * 4ull) {
    const unsigned long long i = base + g;
    bool have = i < total;
    AlignRec a; a.cigar_len = 0; a.cigar_off = 0;
    uint32_t r = 0;
    if (have) {
      r = (uint32_t)(i / slots);
      have = idcov[4 * (size_t)r] != 0u && (uint32_t)(i - (unsigned long long)r * slots) < min(saved[r].n_align, slots);
      if (have) { a = aln[i]; have = a.index_num == index_num && a.part == part; }
    }
    uint32_t bad = 0;
    if (have) {
      if (!(a.has_cigar & 1u)) bad = OTU_E_NOCIG;
      else if (a.ref_num >= ix.n_refs) bad = OTU_E_BADREF;
      else if (a.read_begin1 < 0 || a.ref_begin1 < 0) bad = OTU_E_PAST;
    }
    const bool walk = have && !bad;
    const uint32_t* rec = rd.words; uint32_t cw = 0, readlen = 0;
    unsigned long long pb = 0, qb = 0, ref_end = 0;
    if (walk) {
      rec = rd.words + rd.rec_off[r]; readlen = rd.len[r]; cw = (readlen + 15u) >> 4;
      pb = (unsigned long long)a.read_begin1; qb = ix.ref_off[a.ref_num] + (unsigned long long)a.ref_begin1; ref_end = ix.ref_off[a.ref_num + 1];
    }
    const bool is_long = walk && a.cigar_len > IDCOV_FEW_OPS;
    const uint32_t ncig = walk && !is_long ? a.cigar_len : 0u;
    uint32_t maxc = ncig;
    for (int d = 32; d >= 16; d >>= 1) maxc = max(maxc, (uint32_t)__shfl_xor((int)maxc, d, 64));
    uint32_t n_match = 0, n_miss = 0, n_gap = 0;
    bool past = false;
    // few operations: the 16 lanes of the group stride over the letters of each M run
    for (uint32_t q = 0; q < maxc; q++) {
      if (q < ncig) {
        const uint32_t c = exp_cigar_word(cigar, pool_words, (unsigned long long)a.cigar_off + q), op = c & 0xFu, len = c >> 4;
        if (op == 0u) {
          if (len && (pb + len > readlen || qb + len > ref_end)) past = true;      // an M column outside the read or the reference: what add_otu refuses
          if (pb < readlen) idcov_run(rec, cw, readlen, ix.ref_seq, ref_end, (uint32_t)pb, qb, len, gl, 16u, n_match, n_miss);
          else if (gl == 0u) n_miss += len;
          pb += len; qb += len;
        } else { if (op == 1u) pb += len; else qb += len; if (gl == 0u) n_gap += len; }
      }
    }
    for (int d = 8; d > 0; d >>= 1) { n_match += __shfl_xor((int)n_match, d, 64); n_miss += __shfl_xor((int)n_miss, d, 64); n_gap += __shfl_xor((int)n_gap, d, 64); }
    // many operations: the whole wave on one alignment, an operation per lane, its starts from a scan of the lengths
    const unsigned long long long_m = __ballot(is_long && gl == 0u);
    for (uint32_t gg = 0; gg < 4u; gg++) {
      if (!((long_m >> (16u * gg)) & 1ull)) continue;
      const unsigned long long i2 = base + gg;
      const AlignRec b = aln[i2];
      const uint32_t r2 = (uint32_t)(i2 / slots), rl2 = rd.len[r2], cw2 = (rl2 + 15u) >> 4;
      const uint32_t* rec2 = rd.words + rd.rec_off[r2];
      const unsigned long long re2 = ix.ref_off[b.ref_num + 1];
      unsigned long long pb2 = (unsigned long long)b.read_begin1, qb2 = ix.ref_off[b.ref_num] + (unsigned long long)b.ref_begin1;
      uint32_t m2 = 0, s2 = 0, g2 = 0;
      bool past2 = false;
      for (uint32_t q0 = 0; q0 < b.cigar_len; q0 += 64u) {
        const uint32_t q = q0 + lane;
        const uint32_t c = q < b.cigar_len ? exp_cigar_word(cigar, pool_words, (unsigned long long)b.cigar_off + q) : 0u, op = c & 0xFu, len = c >> 4;
        const uint32_t ra = op == 2u ? 0u : len, fa = op == 1u ? 0u : len;       // letters of the read / of the reference the operation consumes
        const unsigned long long ri = exp_wave_scan(ra), fi = exp_wave_scan(fa);
        const unsigned long long p0 = pb2 + ri - ra;
        bool over = false;
        if (op == 0u) {
          over = len && (p0 + len > rl2 || qb2 + fi > re2);
          if (p0 < rl2) idcov_run(rec2, cw2, rl2, ix.ref_seq, re2, (uint32_t)p0, qb2 + (fi - fa), len, 0u, 1u, m2, s2);
          else s2 += len;
        } else g2 += len;
        if (__ballot(over)) past2 = true;
        pb2 += __shfl(ri, 63, 64); qb2 += __shfl(fi, 63, 64);
      }
      m2 = wave_sum_u32(m2); s2 = wave_sum_u32(s2); g2 = wave_sum_u32(g2);
      if (g == gg) { n_match = m2; n_miss = s2; n_gap = g2; past = past2; }
    }
    if (have && gl == 0u) {
      if (!bad && past) bad = OTU_E_PAST;
      if (bad) atomicAdd(&err[bad], 1u);
      pass[i] = !bad && otu_pass(n_miss, n_gap, n_match, a.read_begin1, a.read_end1, a.readlen, min_id, min_cov) ? 1u : 0u;
    }
  }
}

// meta[i] = {offset, length} of read i's id in the text; excl[i]: the passing slots of the block's reads in front of read i; part[b]: block b's
__global__ void __launch_bounds__(OTU_BLOCK) k_otu_size(uint32_t n, uint32_t slots, const RState* __restrict__ saved, const AlignRec* __restrict__ aln,
                                                        const uint32_t* __restrict__ idcov, const uint8_t* __restrict__ pass, uint32_t index_num, uint32_t part,
                                                        RowsSrc src, uint2* __restrict__ meta, unsigned long long* __restrict__ excl,
                                                        unsigned long long* __restrict__ parts, uint32_t* __restrict__ err) {
  __shared__ unsigned long long s_w[16];
  const uint32_t i = blockIdx.x * OTU_BLOCK + threadIdx.x;
  unsigned long long cnt = 0;
  bool yes = false;
  if (i < n && idcov[4 * (size_t)i] != 0u) {
    yes = true;
    const uint32_t na = min(saved[i].n_align, slots);
    for (uint32_t k = 0; k < na; k++) {
      const AlignRec& a = aln[(size_t)i * slots + k];
      if (a.index_num == index_num && a.part == part && pass[(size_t)i * slots + k]) cnt++;
    }
    if (cnt) {
      // Read::getSeqId on the trimmed header line: up to the first ' ', without the leading '>' / '@'
      const uint32_t h0 = (uint32_t)src.hoff[i], he = fxs_rtrim(src.text, h0, fxs_find_nl(src.text, src.n_text, h0));
      uint32_t ie = h0;
      while (ie < he && fxs_byte(src.text, ie) != ' ') ie++;
      uint32_t is = h0;
      while (is < ie && (fxs_byte(src.text, is) == '>' || fxs_byte(src.text, is) == '@')) is++;
      meta[i] = make_uint2(is, ie - is);
    }
  }
  if (__ballot(yes) && lane_id() == 0) err[OTU_E_ANY] = 1u;       // (every wave that sees one stores the same word)
  unsigned long long total;
  const unsigned long long incl = exp_block_scan(cnt, s_w, total);
  if (i < n) excl[i] = incl - cnt;
  if (threadIdx.x == 0) { parts[blockIdx.x] = total; if (blockIdx.x == 0) parts[gridDim.x] = 0ull; }
}

// the place of entry i of a sequence summed in blocks of OTU_BLOCK (i == n: its total)
__device__ __forceinline__ unsigned long long otu_off(const unsigned long long* __restrict__ excl, const unsigned long long* __restrict__ parts, uint32_t n, uint32_t np, uint32_t i) {
  return i >= n ? parts[np] : parts[i / OTU_BLOCK] + excl[i];
}

__global__ void __launch_bounds__(OTU_BLOCK) k_otu_pairs(uint32_t n, uint32_t slots, const RState* __restrict__ saved, const AlignRec* __restrict__ aln,
                                                         const uint32_t* __restrict__ idcov, const uint8_t* __restrict__ pass, uint32_t index_num, uint32_t part,
                                                         const uint2* __restrict__ meta, const unsigned long long* __restrict__ excl,
                                                         const unsigned long long* __restrict__ parts, uint32_t* __restrict__ keys, uint4* __restrict__ pairs) {
  const uint32_t i = blockIdx.x * OTU_BLOCK + threadIdx.x, np = (n + OTU_BLOCK - 1u) / OTU_BLOCK;
  if (i >= n || idcov[4 * (size_t)i] == 0u) return;
  unsigned long long at = otu_off(excl, parts, n, np, i);
  if (otu_off(excl, parts, n, np, i + 1u) == at) return;
  const uint2 mt = meta[i];
  const uint32_t na = min(saved[i].n_align, slots);
  for (uint32_t k = 0; k < na; k++) {
    const AlignRec& a = aln[(size_t)i * slots + k];
    if (a.index_num == index_num && a.part == part && pass[(size_t)i * slots + k]) { keys[at] = a.ref_num; pairs[at] = make_uint4(a.ref_num, i, mt.x, mt.y); at++; }
  }
}

// ---- the sort --------------------------------------------------------------------------------------------------------------------------
// the lanes of the wave whose digit equals this lane's (an invalid lane: none, itself included)
__device__ __forceinline__ unsigned long long otu_peers(uint32_t digit, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (uint32_t b = 0; b < 8u; b++) {
    const unsigned long long v = __ballot((digit >> b) & 1u);
    m &= ((digit >> b) & 1u) ? v : ~v;
  }
  return valid ? m : 0ull;
}

// hist[d * n_units + u] = the items of unit u (OTU_UNIT consecutive ones, a wave's) whose digit is d
__global__ void __launch_bounds__(256) k_otu_hist(uint32_t n, const uint32_t* __restrict__ keys, uint32_t shift, uint32_t n_units, unsigned long long* __restrict__ hist) {
  __shared__ uint32_t s_cnt[4][256];
  const uint32_t lane = (uint32_t)lane_id(), wv = threadIdx.x >> 6;
  const uint32_t unit = blockIdx.x * 4u + wv;
  uint32_t* const cnt = s_cnt[wv];
  for (uint32_t d = lane; d < 256u; d += 64u) cnt[d] = 0u;
  __threadfence_block();
  if (unit < n_units) {
    for (uint32_t round = 0; round < OTU_UNIT / 64u; round++) {
      const unsigned long long idx = (unsigned long long)unit * OTU_UNIT + round * 64u + lane;
      const bool valid = idx < n;
      const uint32_t digit = valid ? (keys[idx] >> shift) & 255u : 0u;
      const unsigned long long peers = otu_peers(digit, valid);
      const bool leader = valid && (peers & ((1ull << lane) - 1ull)) == 0ull;
      if (leader) cnt[digit] += (uint32_t)__popcll(peers);          // (one lane per digit, a row of counters per wave)
      __threadfence_block();
    }
    for (uint32_t d = lane; d < 256u; d += 64u) hist[(size_t)d * n_units + unit] = cnt[d];
  }
}

// offs: hist after its exclusive scan.  Item idx goes to offs[digit][unit] + the items of the unit in front of it with the same digit: stable.
// The move is staged: the unit's items are first put in LDS in the order of their digits (the counts of the unit are the differences of
// neighbouring offsets, their exclusive sums the digits' places in the stage), then the stage is written out lane after lane, so that the
// items of one digit -- consecutive in the stage -- go to consecutive words of the output whatever the spread of the keys.
// vals_in == nullptr: the values are the items' own places (the first pass)
__global__ void __launch_bounds__(256) k_otu_move(uint32_t n, const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ vals_in, uint32_t shift, uint32_t n_units,
                                                  const unsigned long long* __restrict__ offs, uint32_t* __restrict__ keys_out, uint32_t* __restrict__ vals_out) {
  __shared__ uint32_t s_goff[4][256], s_lst[4][256], s_at[4][256];
  __shared__ uint32_t s_key[4][OTU_UNIT], s_val[4][OTU_UNIT];
  const uint32_t lane = (uint32_t)lane_id(), wv = threadIdx.x >> 6;
  const uint32_t unit = blockIdx.x * 4u + wv;
  uint32_t* const goff = s_goff[wv]; uint32_t* const lst = s_lst[wv]; uint32_t* const at = s_at[wv];
  uint32_t* const skey = s_key[wv]; uint32_t* const sval = s_val[wv];
  if (unit >= n_units) return;
  const size_t n_flat = (size_t)256u * n_units;
  uint32_t carry = 0;
  for (uint32_t d = lane; d < 256u; d += 64u) {
    const size_t f = (size_t)d * n_units + unit;
    const uint32_t g0 = (uint32_t)offs[f], cnt = (f + 1 < n_flat ? (uint32_t)offs[f + 1] : n) - g0;
    const uint32_t incl = wave_scan_add(cnt);
    goff[d] = g0; lst[d] = at[d] = carry + incl - cnt;
    carry += (uint32_t)__shfl((int)incl, 63, 64);
  }
  __threadfence_block();
  for (uint32_t round = 0; round < OTU_UNIT / 64u; round++) {
    const unsigned long long idx = (unsigned long long)unit * OTU_UNIT + round * 64u + lane;
    const bool valid = idx < n;
    const uint32_t key = valid ? keys_in[idx] : 0u, digit = (key >> shift) & 255u;
    const uint32_t val = valid ? (vals_in ? vals_in[idx] : (uint32_t)idx) : 0u;
    const unsigned long long peers = otu_peers(digit, valid);
    const uint32_t rank = (uint32_t)__popcll(peers & ((1ull << lane) - 1ull));
    const uint32_t first = valid ? at[digit] : 0u;
    __threadfence_block();                                          // (all have read the counter before its one writer moves it on)
    if (valid && rank == 0u) at[digit] = first + (uint32_t)__popcll(peers);
    if (valid && first + rank < OTU_UNIT) { skey[first + rank] = key; sval[first + rank] = val; }
    __threadfence_block();
  }
  const unsigned long long u0 = (unsigned long long)unit * OTU_UNIT;
  const uint32_t mine = (uint32_t)min((unsigned long long)OTU_UNIT, (unsigned long long)n - u0);
  for (uint32_t j = lane; j < mine; j += 64u) {
    const uint32_t key = skey[j], digit = (key >> shift) & 255u;
    const unsigned long long dst = (unsigned long long)goff[digit] + (j - lst[digit]);
    if (dst < n) { keys_out[dst] = key; vals_out[dst] = sval[j]; }
  }
}

__global__ void k_otu_iota(uint32_t n, uint32_t* __restrict__ vals) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) vals[i] = i;
}

// ---- writing ---------------------------------------------------------------------------------------------------------------------------
// over the sorted pairs k (pair perm[k], key keys[k]): wexcl / wparts: the bytes in front of k (id + '\t', the last member of a group: the
// id alone); gexcl / gparts: the groups that start in front of k
__global__ void __launch_bounds__(OTU_BLOCK) k_otu_wsize(uint32_t m, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm, const uint4* __restrict__ pairs,
                                                         unsigned long long* __restrict__ wexcl, unsigned long long* __restrict__ wparts,
                                                         unsigned long long* __restrict__ gexcl, unsigned long long* __restrict__ gparts) {
  __shared__ unsigned long long s_w[16];
  const uint32_t k = blockIdx.x * OTU_BLOCK + threadIdx.x;
  unsigned long long bytes = 0, starts = 0;
  if (k < m) {
    const uint32_t key = keys[k];
    bytes = (unsigned long long)pairs[perm[k]].w + ((k + 1u < m && keys[k + 1u] == key) ? 1ull : 0ull);
    starts = (k == 0u || keys[k - 1u] != key) ? 1ull : 0ull;
  }
  unsigned long long total;
  const unsigned long long wi = exp_block_scan(bytes, s_w, total);
  if (k < m) wexcl[k] = wi - bytes;
  if (threadIdx.x == 0) { wparts[blockIdx.x] = total; if (blockIdx.x == 0) wparts[gridDim.x] = 0ull; }
  const unsigned long long gi = exp_block_scan(starts, s_w, total);
  if (k < m) gexcl[k] = gi - starts;
  if (threadIdx.x == 0) { gparts[blockIdx.x] = total; if (blockIdx.x == 0) gparts[gridDim.x] = 0ull; }
}

__global__ void __launch_bounds__(256) k_otu_write(uint32_t m, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm, const uint4* __restrict__ pairs,
                                                   const uint8_t* __restrict__ text, const unsigned long long* __restrict__ wexcl,
                                                   const unsigned long long* __restrict__ wparts, uint8_t* __restrict__ out) {
  __shared__ __align__(16) uint32_t s_win[4][ROWS_WINDOW / 4 + 16];
  const int lane = lane_id();
  const uint32_t np = (m + OTU_BLOCK - 1u) / OTU_BLOCK;
  const uint32_t n_chunks = (m + 63u) >> 6, n_waves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t chunk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); chunk < n_chunks; chunk += n_waves) {
    const uint32_t k = chunk * 64u + (uint32_t)lane;
    const unsigned long long o0 = otu_off(wexcl, wparts, m, np, min(k, m)), o1 = otu_off(wexcl, wparts, m, np, min(k + 1u, m));
    unsigned long long todo = __ballot(o1 != o0);
    if (!todo) continue;
    const int r_first = __ffsll((long long)todo) - 1, r_last = 63 - __clzll((long long)todo);
    RowsWave w;
    w.win = s_win[threadIdx.x >> 6]; w.win8 = reinterpret_cast<uint8_t*>(w.win); w.out = out; w.lane = lane;
    w.first = __shfl(o0, r_first);
    const unsigned long long last = __shfl(o1, r_last);
    w.wbase = w.first & ~3ull; w.pos = w.first;
    while (todo) {
      const uint32_t kk = chunk * 64u + (uint32_t)(__ffsll((long long)todo) - 1);
      todo &= todo - 1ull;
      const uint4 p = pairs[perm[kk]];
      w.text(text, p.z, p.w, false);
      if (kk + 1u < m && keys[kk + 1u] == keys[kk]) ROWS_LIT(w, "\t");
    }
    w.flush();
    // what is left in the window: the bytes of the range's last dword, which the next wave's ids may share
    if (lane == 0) for (unsigned long long b = max(w.wbase, w.first); b < last; b++) out[b] = w.win8[b - w.wbase];
    __threadfence_block();
  }
}

// a group starts at sorted pair k: its reference, its first byte and, in gstart[], k
__global__ void __launch_bounds__(OTU_BLOCK) k_otu_groups(uint32_t m, const uint32_t* __restrict__ keys, const unsigned long long* __restrict__ wexcl,
                                                          const unsigned long long* __restrict__ wparts, const unsigned long long* __restrict__ gexcl,
                                                          const unsigned long long* __restrict__ gparts, OtuGroup* __restrict__ groups, uint32_t* __restrict__ gstart) {
  const uint32_t k = blockIdx.x * OTU_BLOCK + threadIdx.x, np = (m + OTU_BLOCK - 1u) / OTU_BLOCK;
  if (k >= m || (k != 0u && keys[k - 1u] == keys[k])) return;
  const unsigned long long gi = otu_off(gexcl, gparts, m, np, k);
  groups[gi].ref_num = keys[k]; groups[gi].off = otu_off(wexcl, wparts, m, np, k);
  gstart[gi] = k;
}
__global__ void k_otu_gcount(uint32_t n_groups, uint32_t m, const uint32_t* __restrict__ gstart, OtuGroup* __restrict__ groups) {
  const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi < n_groups) groups[gi].n_reads = (gi + 1u < n_groups ? gstart[gi + 1u] : m) - gstart[gi];
}

}  // namespace smr
