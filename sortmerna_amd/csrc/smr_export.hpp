// smr_export.hpp -- the inverse of smr_import.hpp: the stored per-read state of a batch (RState / AlignRec / the CIGAR pool, the id / coverage
// counters) written out as Read::toBinString records, back to back, with an array of n + 1 byte offsets.  The byte layout is the one at the
// top of smr_import.hpp; record_of in smr_engine.hip writes the same bytes one read at a time on the host.
//
// Sizing (k_export_size, k_export_scan, k_export_offsets): a read without alignments has no record (length 0), any other 61 bytes + per
// alignment 47 + 4 * its CIGAR words.  k_export_size leaves in off[i + 1] the inclusive sum of the lengths inside its block of 1024 reads (two
// wave_scan_add per wave: the low 24 bits and the rest of a length, so nothing overflows 32 bits in a scan step) and the block's sum in part[];
// k_export_scan, one block, turns part[] into its exclusive sums; k_export_offsets adds them.  All offsets are 64 bit.
//
// Writing (k_export_state): neither records nor fields are 4-byte aligned, so neighbouring records share a dword and so do the byte ranges of
// neighbouring waves.  A wave takes 64 consecutive reads, whose records are ONE contiguous byte range [off[first], off[last + 1]), and streams
// it through a window of LDS that starts on a dword of the output:
//   * records of up to EXP_SMALL bytes: as many consecutive ones as fit the window at once, every lane writes ITS record into LDS (bytes and
//     unaligned words are LDS's business), then the wave stores the window's whole dwords, lane after lane: coalesced dword stores;
//   * a longer record: the wave goes through its alignments, lane k & 63 puts the fixed fields of alignment k into the window, all lanes the
//     words of a CIGAR of up to 64 words; a longer CIGAR does not pass through LDS: the window is stored first, then every output dword is put
//     together from two neighbouring pool words by a byte funnel shift (the inverse of imp_u32) and stored directly;
//   * the bytes behind the last whole dword stay in the window (its first dword) and are completed by what follows.
// Who stores a dword that is shared: inside a wave's range nobody shares, every dword is completed in the window and stored once.  The first
// and the last dword of the range can hold bytes of the neighbouring waves' records: of such a dword a wave stores ITS bytes only, as bytes
// (exp_flush for the first, the end of the chunk for the last).  So no dword store ever touches a byte that is not the storing wave's, and
// nothing is stored at or behind off[n].
#pragma once

namespace smr {

#define EXP_HEADER 61u
#define EXP_ALN_FIXED 47u
#define EXP_WINDOW 8192u        // bytes of LDS window per wave
#define EXP_SMALL 512u          // records up to this many bytes are written by one lane each
#define EXP_SIZE_BLOCK 1024u

// ---- sizing ----------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long exp_record_len(const RState* __restrict__ saved, const AlignRec* __restrict__ saved_aln, uint32_t slots, uint32_t i) {
  const uint32_t na = min(saved[i].n_align, slots);
  if (na == 0) return 0ull;
  unsigned long long L = EXP_HEADER;
  for (uint32_t k = 0; k < na; k++) {
    const AlignRec& a = saved_aln[(size_t)i * slots + k];
    L += EXP_ALN_FIXED + (a.has_cigar ? 4ull * a.cigar_len : 0ull);
  }
  return L;
}
// inclusive sum over the lanes of a wave, v < 2^50
__device__ __forceinline__ unsigned long long exp_wave_scan(unsigned long long v) {
  return (unsigned long long)wave_scan_add((uint32_t)v & 0xFFFFFFu) + ((unsigned long long)wave_scan_add((uint32_t)(v >> 24)) << 24);
}
// inclusive sum over a block of up to 1024 threads (every thread calls it); total: the block's sum.  s_w: 16 u64 of LDS
__device__ __forceinline__ unsigned long long exp_block_scan(unsigned long long v, unsigned long long* s_w, unsigned long long& total) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nwv = (blockDim.x + 63u) >> 6;
  unsigned long long incl = exp_wave_scan(v);
  __syncthreads();                                    // (s_w of the previous call has been read)
  if (lane == 63u) s_w[wv] = incl;
  __syncthreads();
  unsigned long long before = 0, all = 0;
  for (uint32_t q = 0; q < nwv; q++) { const unsigned long long t = s_w[q]; if (q < wv) before += t; all += t; }
  total = all;
  return incl + before;
}
__global__ void __launch_bounds__(EXP_SIZE_BLOCK) k_export_size(uint32_t n, uint32_t slots, const RState* __restrict__ saved, const AlignRec* __restrict__ saved_aln,
                                                                unsigned long long* __restrict__ off, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long s_w[16];
  const uint32_t i = blockIdx.x * EXP_SIZE_BLOCK + threadIdx.x;
  const unsigned long long L = i < n ? exp_record_len(saved, saved_aln, slots, i) : 0ull;
  unsigned long long total;
  const unsigned long long incl = exp_block_scan(L, s_w, total);
  if (i < n) off[(size_t)i + 1] = incl;
  if (threadIdx.x == 0) { part[blockIdx.x] = total; if (blockIdx.x == 0) off[0] = 0ull; }
}
// part[0 .. np) -> its exclusive sums, in place (one block)
__global__ void __launch_bounds__(EXP_SIZE_BLOCK) k_export_scan(unsigned long long* __restrict__ part, uint32_t np) {
  __shared__ unsigned long long s_w[16];
  unsigned long long carry = 0;
  for (uint32_t b = 0; b < np; b += EXP_SIZE_BLOCK) {
    const uint32_t q = b + threadIdx.x;
    const unsigned long long v = q < np ? part[q] : 0ull;
    unsigned long long total;
    const unsigned long long incl = exp_block_scan(v, s_w, total);
    if (q < np) part[q] = carry + incl - v;
    carry += total;
  }
}
__global__ void __launch_bounds__(EXP_SIZE_BLOCK) k_export_offsets(uint32_t n, unsigned long long* __restrict__ off, const unsigned long long* __restrict__ part) {
  const uint32_t i = blockIdx.x * EXP_SIZE_BLOCK + threadIdx.x;
  if (i < n && blockIdx.x) off[(size_t)i + 1] += part[blockIdx.x];
}

// ---- writing -----------------------------------------------------------------------------------------------------------------------------
// (p: any byte of the LDS window; the compiler picks the stores the alignment it can prove allows)
__device__ __forceinline__ uint8_t* exp_put32(uint8_t* p, uint32_t v) { __builtin_memcpy(p, &v, 4); return p + 4; }
__device__ __forceinline__ uint8_t* exp_put16(uint8_t* p, uint16_t v) { __builtin_memcpy(p, &v, 2); return p + 2; }
__device__ __forceinline__ uint8_t* exp_put64(uint8_t* p, unsigned long long v) { return exp_put32(exp_put32(p, (uint32_t)v), (uint32_t)(v >> 32)); }
// the 61 bytes in front of the alignments; L: the record's length
__device__ __forceinline__ uint8_t* exp_header(uint8_t* p, const RState& s, const uint32_t* __restrict__ ic, uint32_t num_alignments, uint32_t na, unsigned long long L) {
  p = exp_put32(p, s.lastIndex); p = exp_put32(p, s.lastPart);
  for (int k = 0; k < 4; k++) p = exp_put32(p, ic ? ic[k] : 0u);
  *p++ = s.is_done; *p++ = s.is_hit; *p++ = 0;                      // (null_align_output)
  p = exp_put16(p, s.max_SW_count); p = exp_put32(p, num_alignments); p = exp_put32(p, s.hit_seeds);
  p = exp_put64(p, L - 45u); p = exp_put32(p, s.min_index); p = exp_put32(p, s.max_index);
  return exp_put64(p, (unsigned long long)na);
}
// the 31 bytes behind an alignment's CIGAR
__device__ __forceinline__ uint8_t* exp_aln_tail(uint8_t* p, const AlignRec& a) {
  p = exp_put32(p, a.ref_num); p = exp_put32(p, (uint32_t)a.ref_begin1); p = exp_put32(p, (uint32_t)a.ref_end1); p = exp_put32(p, (uint32_t)a.read_begin1);
  p = exp_put32(p, (uint32_t)a.read_end1); p = exp_put32(p, a.readlen);
  p = exp_put16(p, a.score1); p = exp_put16(p, a.part); p = exp_put16(p, a.index_num);
  *p++ = a.strand;
  return p;
}
__device__ __forceinline__ uint32_t exp_cigar_word(const uint32_t* __restrict__ cigar, unsigned long long pool_words, unsigned long long w) { return w < pool_words ? cigar[w] : 0u; }

// Stores the whole dwords of the window, which holds the output bytes [wbase, pos) (wbase on a dword), and moves what is left behind them to
// the window's start.  first: the first byte of the wave's range; of the dword it lies in, only the bytes from `first` on are the wave's.
__device__ __forceinline__ void exp_flush(uint32_t* __restrict__ win, uint8_t* __restrict__ out, unsigned long long& wbase, unsigned long long pos, unsigned long long first, int lane) {
  __threadfence_block();
  const uint32_t nd = (uint32_t)((pos - wbase) >> 2);
  uint32_t* const out32 = reinterpret_cast<uint32_t*>(out);
  for (uint32_t j = (uint32_t)lane; j < nd; j += 64u) {
    const uint32_t v = win[j];
    const unsigned long long b = wbase + 4ull * j;
    if (b >= first) out32[b >> 2] = v;
    else for (uint32_t q = (uint32_t)(first - b); q < 4u; q++) out[b + q] = (uint8_t)(v >> (8u * q));
  }
  const uint32_t rest = (pos & 3ull) ? win[nd] : 0u;
  __threadfence_block();
  if (lane == 0 && nd) win[0] = rest;
  __threadfence_block();
  wbase += 4ull * nd;
}

__global__ void __launch_bounds__(256) k_export_state(uint32_t n, uint32_t slots, const RState* __restrict__ saved, const AlignRec* __restrict__ saved_aln, const uint32_t* __restrict__ cigar,
                                                      unsigned long long pool_words, const uint32_t* __restrict__ idcov, uint32_t num_alignments,
                                                      const unsigned long long* __restrict__ off, uint8_t* __restrict__ out) {
  __shared__ __align__(16) uint32_t s_win[4][EXP_WINDOW / 4 + 16];
  const int lane = lane_id();
  uint32_t* const win = s_win[threadIdx.x >> 6];
  uint8_t* const win8 = reinterpret_cast<uint8_t*>(win);
  uint32_t* const out32 = reinterpret_cast<uint32_t*>(out);
  const uint32_t n_chunks = (n + 63u) >> 6, n_waves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t chunk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); chunk < n_chunks; chunk += n_waves) {
    const uint32_t i = chunk * 64u + (uint32_t)lane;
    const unsigned long long o0 = off[min(i, n)], o1 = off[min(i + 1u, n)], L = o1 - o0;      // (a lane behind the batch: an empty record at its end)
    unsigned long long m = __ballot(L != 0);
    if (!m) continue;
    const int r_first = __ffsll((long long)m) - 1, r_last = 63 - __clzll((long long)m);
    const unsigned long long first = __shfl(o0, r_first), last = __shfl(o1, r_last);      // the wave's bytes: [first, last)
    unsigned long long wbase = first & ~3ull;                                             // the window holds [wbase, pos)
    while (m) {
      const int r = __ffsll((long long)m) - 1;
      const unsigned long long ro = __shfl(o0, r), rL = __shfl(L, r);
      if (rL <= EXP_SMALL) {
        // the records from r on that are small and end inside the window (the first one does: the window holds less than a dword)
        const bool fits = lane >= r && L <= EXP_SMALL && o1 - wbase <= EXP_WINDOW;
        const unsigned long long nf = ~__ballot(fits) & ~((1ull << r) - 1ull);
        const int e = nf ? __ffsll((long long)nf) - 1 : 64;                               // records [r, e)
        if (lane >= r && lane < e && L) {
          const RState s = saved[i];
          const uint32_t na = min(s.n_align, slots);
          uint8_t* p = exp_header(win8 + (o0 - wbase), s, idcov ? idcov + 4 * (size_t)i : nullptr, num_alignments, na, L);
          for (uint32_t k = 0; k < na; k++) {
            const AlignRec a = saved_aln[(size_t)i * slots + k];
            const uint32_t cl = a.has_cigar ? a.cigar_len : 0u;
            p = exp_put64(p, 4ull * cl + (EXP_ALN_FIXED - 8u)); p = exp_put64(p, (unsigned long long)cl);
            for (uint32_t j = 0; j < cl; j++) p = exp_put32(p, exp_cigar_word(cigar, pool_words, (unsigned long long)a.cigar_off + j));
            p = exp_aln_tail(p, a);
          }
        }
        const unsigned long long pos = __shfl(o1, e - 1);
        exp_flush(win, out, wbase, pos, first, lane);
        m &= e < 64 ? ~((1ull << e) - 1ull) : 0ull;
      } else {
        // one long record, the whole wave on it
        m &= m - 1;
        const uint32_t ri = chunk * 64u + (uint32_t)r;
        const RState s = saved[ri];
        const uint32_t na = min(s.n_align, slots);
        unsigned long long pos = ro;
        if (lane == 0) exp_header(win8 + (pos - wbase), s, idcov ? idcov + 4 * (size_t)ri : nullptr, num_alignments, na, rL);
        pos += EXP_HEADER;
        for (uint32_t k = 0; k < na; k++) {
          const AlignRec a = saved_aln[(size_t)ri * slots + k];
          const uint32_t cl = a.has_cigar ? a.cigar_len : 0u;
          const bool direct = cl > 64u;
          if (pos - wbase + EXP_ALN_FIXED + (direct ? 0ull : 4ull * cl) > EXP_WINDOW) exp_flush(win, out, wbase, pos, first, lane);
          if ((uint32_t)lane == (k & 63u)) exp_put64(exp_put64(win8 + (pos - wbase), 4ull * cl + (EXP_ALN_FIXED - 8u)), (unsigned long long)cl);
          pos += 16u;
          if (direct) {
            // the window holds [wbase, pos): fewer than four bytes once it is flushed (the record's header lies in front, so the first
            // dword of the wave's range has been stored).  Output dword j takes its low sh bytes from the word before: the window's, or pool word j - 1
            exp_flush(win, out, wbase, pos, first, lane);
            const uint32_t sh = 8u * (uint32_t)(pos & 3ull), head = win[0];
            const unsigned long long w0 = a.cigar_off, d0 = wbase >> 2;
            for (uint32_t j = (uint32_t)lane; j < cl; j += 64u) {
              const uint32_t hi = exp_cigar_word(cigar, pool_words, w0 + j);
              if (sh) {
                const uint32_t lo = j ? exp_cigar_word(cigar, pool_words, w0 + j - 1u) >> (32u - sh) : head & ((1u << sh) - 1u);
                out32[d0 + j] = lo | (hi << sh);
              } else out32[d0 + j] = hi;
            }
            __threadfence_block();
            if (lane == 0 && sh) win[0] = exp_cigar_word(cigar, pool_words, w0 + cl - 1u) >> (32u - sh);
            __threadfence_block();
            wbase += 4ull * cl;
          } else {
            for (uint32_t j = (uint32_t)lane; j < cl; j += 64u) exp_put32(win8 + (pos - wbase) + 4u * j, exp_cigar_word(cigar, pool_words, (unsigned long long)a.cigar_off + j));
          }
          pos += 4ull * cl;
          if ((uint32_t)lane == (k & 63u)) exp_aln_tail(win8 + (pos - wbase), a);
          pos += EXP_ALN_FIXED - 16u;
        }
        exp_flush(win, out, wbase, pos, first, lane);
      }
    }
    // what is left in the window: the bytes of the range's last dword, which the next wave's record may share
    if (lane == 0) for (unsigned long long b = max(wbase, first); b < last; b++) out[b] = win8[b - wbase];
    __threadfence_block();
  }
}

}  // namespace smr
