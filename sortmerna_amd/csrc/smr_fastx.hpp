// smr_fastx.hpp -- K1 of SURVEY.md 2: FASTA/FASTQ text parsed and 2-bit packed on the device.  The definition of every result is the host
// parser of smr_reads.cpp (list_range, pack_piece, load_fastx_impl), which replaces Readfeed::next() -> Read(readstr) -> Read::init()
// (/root/reference/src/sortmerna/readfeed.cpp:776-873, read.cpp:264-347; nt_table: include/common.hpp:68-77): letters outside ACGTU become 0
// and their position is kept in the mask words (Read::ambiguous_nt).  The kernels take the whole text [0, n) in device memory (n < 2^32 - 64,
// offsets are 32 bit), `first` = the first byte that is neither '\n' nor '\r' (the host looks for it: a handful of bytes) and the format.
//
// Lines.  Line 0 starts at `first`; every '\n' at p in [first, n - 1) starts a line at p + 1 (a final '\n' starts none).
//   k_fx_count    a lane takes 16 bytes as one dwordx4, a block a tile of FX_TILE bytes: newlines per tile
//   k_fx_scan     one block: the per-tile (per-block) counts to their exclusive sums, the total into tot[]
//   k_fx_lines    the same masks again: line_start[1 + rank] = p + 1; line_start[NL] = one past the last line's end + 1, so that line j ends
//                 (its '\n', or n) at line_start[j + 1] - 1 for every j
// Records.  One thread per line, blocks of FX_LBLOCK lines, two sums over the lines at once: headers and letters.
//   k_fx_classify FASTA: a line is a header iff its first byte is '>', every other line is sequence (rtrim'med length).  FASTQ: line 4k is a
//                 header, 4k + 1 the sequence.  Regular FASTQ: every line 4k begins with '@' up to the last record, the record
//                 count is whole, what follows is lines that are empty or one '\r'.  The kernel raises FXT_FLAG for a line 4k that is neither
//                 '@...' nor blank and keeps the last non-blank line and the first blank line 4k; k_fx_records draws the conclusion.
//   k_fx_scan     headers and letters per block to exclusive sums; totals = records, total_len
//   k_fx_records  lcum[j] := letters in front of line j (whole text); a header line of record r leaves hdr_line[r] = j, rcum[r] = lcum[j]
//   k_fx_reclen   per record: len = rcum[r + 1] - rcum[r], hdr_off, seq_off, words = (len + 15) / 16 + (len + 31) / 32 summed per block;
//                 min / max of len
//   k_fx_scan     words per block to exclusive sums; total words
// (the host reads tot[] here: the one D2H it needs to reserve the batch)
// Pack.  k_fx_pack: a wave takes 64 consecutive records; a unit = 32 letters of a record = two code words and one mask word, the units of
//   the 64 records are numbered through (wave_scan_add) and dealt to the lanes, so a 5 000-letter record is packed by the whole wave and 64
//   150-letter reads keep 320 units busy.  A unit whose letters lie on one line (every FASTQ unit, most FASTA units) reads them as aligned
//   dwords and shifts by the byte phase of its start; a unit that spans lines gathers them piece by piece.  Every word is put together in
//   registers and stored once; nothing is read at or behind n into a result (the text buffer is padded by 64 bytes for the aligned loads).
#pragma once

namespace smr {

#define FX_BLOCK 256u
#define FX_TILE (FX_BLOCK * 16u)      // text bytes per block of k_fx_count / k_fx_lines, which is also the most lines a block can find
#define FX_LBLOCK 1024u               // lines / records per block of the record kernels
enum { FXT_NEWLINES = 0, FXT_FLAG, FXT_LAST_NONBLANK, FXT_FIRST_BLANK_HDR, FXT_RECORDS, FXT_TOTAL_LEN, FXT_MIN_LEN, FXT_MAX_LEN, FXT_WORDS, FXT_COUNT = 16 };

// inclusive sum over a block of up to 1024 threads (every thread calls it); total: the block's sum.  s_w: 16 words of LDS
__device__ __forceinline__ uint32_t fx_block_scan(uint32_t v, uint32_t* s_w, uint32_t& total) {
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, nwv = (blockDim.x + 63u) >> 6;
  const uint32_t incl = wave_scan_add(v);
  __syncthreads();                                    // (s_w of the previous call has been read)
  if (lane == 63u) s_w[wv] = incl;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t q = 0; q < nwv; q++) { const uint32_t t = s_w[q]; if (q < wv) before += t; all += t; }
  total = all;
  return incl + before;
}
// bit k: byte k of the 16 at `base` (16-aligned) is a '\n' that starts a line
__device__ __forceinline__ uint32_t fx_nl_mask(const uint8_t* __restrict__ text, uint32_t n, uint32_t first, unsigned long long base) {
  if (base >= n) return 0u;
  const uint4 v = *reinterpret_cast<const uint4*>(text + base);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t m = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint32_t x = w[q] ^ 0x0A0A0A0Au;
    const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);      // 0x80 in every byte of x that is 0
    m |= ((((z >> 7) * 0x00204081u) >> 21) & 0xFu) << (4 * q);
  }
  const uint32_t b = (uint32_t)base;
  const uint32_t lo = first > b ? min(first - b, 16u) : 0u, hi = n - 1u > b ? min(n - 1u - b, 16u) : 0u;      // positions [first, n - 1)
  return m & ~((1u << lo) - 1u) & ((1u << hi) - 1u);
}

__global__ void __launch_bounds__(FX_BLOCK) k_fx_count(const uint8_t* __restrict__ text, uint32_t n, uint32_t first, uint32_t* __restrict__ part) {
  __shared__ uint32_t s_w[16];
  const unsigned long long base = (unsigned long long)blockIdx.x * FX_TILE + threadIdx.x * 16u;
  uint32_t total;
  fx_block_scan((uint32_t)__popc(fx_nl_mask(text, n, first, base)), s_w, total);
  if (threadIdx.x == 0) part[blockIdx.x] = total;
}
// a[0 .. np) (and b[0 .. np) when given) -> exclusive sums in place, the totals to tot[ia] (tot[ib]).  One block.
__global__ void __launch_bounds__(FX_LBLOCK) k_fx_scan(uint32_t* __restrict__ a, uint32_t* __restrict__ b, uint32_t np, uint32_t* __restrict__ tot, uint32_t ia, uint32_t ib) {
  __shared__ uint32_t s_w[16];
  uint32_t ca = 0, cb = 0;
  for (uint32_t o = 0; o < np; o += FX_LBLOCK) {
    const uint32_t q = o + threadIdx.x;
    const uint32_t va = q < np ? a[q] : 0u, vb = (b && q < np) ? b[q] : 0u;
    uint32_t ta, tb;
    const uint32_t sa = fx_block_scan(va, s_w, ta), sb = fx_block_scan(vb, s_w, tb);
    if (q < np) { a[q] = ca + sa - va; if (b) b[q] = cb + sb - vb; }
    ca += ta; cb += tb;
  }
  if (threadIdx.x == 0) { tot[ia] = ca; if (b) tot[ib] = cb; }
}
__global__ void __launch_bounds__(FX_BLOCK) k_fx_lines(const uint8_t* __restrict__ text, uint32_t n, uint32_t first, const uint32_t* __restrict__ part,
                                                       const uint32_t* __restrict__ tot, uint32_t* __restrict__ line_start) {
  __shared__ uint32_t s_w[16];
  const unsigned long long base = (unsigned long long)blockIdx.x * FX_TILE + threadIdx.x * 16u;
  uint32_t m = fx_nl_mask(text, n, first, base), total;
  const uint32_t cnt = (uint32_t)__popc(m);
  uint32_t at = 1u + part[blockIdx.x] + fx_block_scan(cnt, s_w, total) - cnt;
  while (m) { const uint32_t k = (uint32_t)__ffs((int)m) - 1u; m &= m - 1u; line_start[at++] = (uint32_t)base + k + 1u; }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    line_start[0] = first;
    line_start[tot[FXT_NEWLINES] + 1u] = text[n - 1u] == '\n' ? n : n + 1u;
  }
}

__device__ __forceinline__ bool fx_trimmed(uint8_t c) { return c == '\r' || c == ' ' || c == '\t'; }      // rtrim of smr_reads.cpp

// lrec[j] = (headers among the block's lines up to j) << 1 | line j is a header; lcum[j] = letters of the block's lines in front of j
__global__ void __launch_bounds__(FX_LBLOCK) k_fx_classify(const uint8_t* __restrict__ text, uint32_t fastq, uint32_t nl, const uint32_t* __restrict__ line_start,
                                                           uint32_t* __restrict__ lrec, uint32_t* __restrict__ lcum, uint32_t* __restrict__ part_h, uint32_t* __restrict__ part_l,
                                                           uint32_t* __restrict__ tot) {
  __shared__ uint32_t s_w[16];
  __shared__ uint32_t s_last, s_blank;
  if (threadIdx.x == 0) { s_last = 0u; s_blank = ~0u; }
  __syncthreads();
  const uint32_t j = blockIdx.x * FX_LBLOCK + threadIdx.x;
  uint32_t hdr = 0, letters = 0;
  bool bad = false, nonblank = false, blank_hdr = false;
  if (j < nl) {
    const uint32_t s = line_start[j], e = line_start[j + 1u] - 1u;
    uint32_t le = e;
    while (le > s && fx_trimmed(text[le - 1u])) le--;
    const uint8_t c0 = text[s];                                   // (s < n; an empty line's first byte is its '\n')
    const bool blank = e == s || (e == s + 1u && c0 == '\r');
    if (!fastq) { hdr = c0 == '>'; letters = hdr ? 0u : le - s; }
    else {
      const uint32_t q = j & 3u;
      if (q == 0u) { hdr = c0 == '@'; blank_hdr = !hdr && blank; bad = !hdr && !blank; }
      else if (q == 1u) letters = le - s;
      nonblank = !blank;
    }
  }
  const unsigned long long m_bad = __ballot(bad), m_nb = __ballot(nonblank), m_bh = __ballot(blank_hdr);
  if ((threadIdx.x & 63u) == 0u) {
    const uint32_t j0 = j;                                        // the wave's first line
    if (m_bad) atomicOr(&tot[FXT_FLAG], 1u);
    if (m_nb) atomicMax(&s_last, j0 + 64u - (uint32_t)__clzll((long long)m_nb));
    if (m_bh) atomicMin(&s_blank, j0 + (uint32_t)__ffsll((long long)m_bh) - 1u);
  }
  uint32_t th, tl;
  const uint32_t ih = fx_block_scan(hdr, s_w, th), il = fx_block_scan(letters, s_w, tl);
  if (j < nl) { lrec[j] = (ih << 1) | hdr; lcum[j] = il - letters; }
  if (threadIdx.x == 0) {                                         // (the barriers of the scans lie between the waves' atomics and these reads)
    part_h[blockIdx.x] = th; part_l[blockIdx.x] = tl;
    if (s_last) atomicMax(&tot[FXT_LAST_NONBLANK], s_last);
    if (s_blank != ~0u) atomicMin(&tot[FXT_FIRST_BLANK_HDR], s_blank);
  }
}
__global__ void __launch_bounds__(FX_LBLOCK) k_fx_records(uint32_t fastq, uint32_t nl, const uint32_t* __restrict__ lrec, uint32_t* __restrict__ lcum, const uint32_t* __restrict__ part_h,
                                                          const uint32_t* __restrict__ part_l, uint32_t* __restrict__ hdr_line, uint32_t* __restrict__ rcum, uint32_t* __restrict__ tot) {
  const uint32_t j = blockIdx.x * FX_LBLOCK + threadIdx.x;
  if (j >= nl) return;
  const uint32_t g = part_l[blockIdx.x] + lcum[j], h = lrec[j];
  lcum[j] = g;
  if (h & 1u) { const uint32_t r = part_h[blockIdx.x] + (h >> 1) - 1u; hdr_line[r] = j; rcum[r] = g; }
  if (j == 0u) {
    const uint32_t R = tot[FXT_RECORDS], L = tot[FXT_TOTAL_LEN];
    hdr_line[R] = nl; rcum[R] = L; lcum[nl] = L;
    if (fastq) {
      const uint32_t fb = tot[FXT_FIRST_BLANK_HDR];
      if (tot[FXT_LAST_NONBLANK] > fb || (fb == ~0u && (nl & 3u))) atomicOr(&tot[FXT_FLAG], 2u);      // text behind the last record / a cut last record
    }
  }
}
__device__ __forceinline__ uint32_t fx_words(uint32_t len) { return (len + 15u) / 16u + (len + 31u) / 32u; }
// rwi[r] = words of the block's records in front of r
__global__ void __launch_bounds__(FX_LBLOCK) k_fx_reclen(uint32_t n, const uint32_t* __restrict__ line_start, const uint32_t* __restrict__ hdr_line, const uint32_t* __restrict__ rcum,
                                                         uint32_t* __restrict__ tot, uint32_t* __restrict__ rlen, uint32_t* __restrict__ rwi, uint32_t* __restrict__ part_w,
                                                         unsigned long long* __restrict__ hoff, unsigned long long* __restrict__ soff) {
  __shared__ uint32_t s_w[16];
  __shared__ uint32_t s_min, s_max;
  if (threadIdx.x == 0) { s_min = ~0u; s_max = 0u; }
  __syncthreads();
  const uint32_t r = blockIdx.x * FX_LBLOCK + threadIdx.x, R = tot[FXT_RECORDS];
  uint32_t len = 0, words = 0, lo = ~0u, hi = 0u;
  if (r < R) {
    len = rcum[r + 1u] - rcum[r]; words = fx_words(len); lo = hi = len;
    const uint32_t j = hdr_line[r];
    rlen[r] = len; hoff[r] = line_start[j]; soff[r] = min(line_start[j + 1u], n);
  }
  for (int d = 1; d < 64; d <<= 1) { lo = min(lo, (uint32_t)__shfl_xor((int)lo, d)); hi = max(hi, (uint32_t)__shfl_xor((int)hi, d)); }
  if ((threadIdx.x & 63u) == 0u && lo != ~0u) { atomicMin(&s_min, lo); atomicMax(&s_max, hi); }
  uint32_t tw;
  const uint32_t iw = fx_block_scan(words, s_w, tw);
  if (r < R) rwi[r] = iw - words;
  if (threadIdx.x == 0) {
    part_w[blockIdx.x] = tw;
    if (s_min != ~0u) { atomicMin(&tot[FXT_MIN_LEN], s_min); atomicMax(&tot[FXT_MAX_LEN], s_max); }
  }
}

// code_of of smr_reads.cpp: ACGTUacgtu -> 0..3, anything else 4
__device__ __forceinline__ uint32_t fx_code(uint32_t c) {
  const uint32_t u = c & 0xDFu;
  const bool ok = u == 'A' || u == 'C' || u == 'G' || u == 'T' || u == 'U';
  return ok ? (((u >> 1) & 3u) ^ ((u >> 2) & 1u)) : 4u;
}
__global__ void __launch_bounds__(256) k_fx_pack(const uint8_t* __restrict__ text, uint32_t n_rec, const uint32_t* __restrict__ line_start, const uint32_t* __restrict__ lcum,
                                                 const uint32_t* __restrict__ hdr_line, const uint32_t* __restrict__ rcum, const uint32_t* __restrict__ rlen, const uint32_t* __restrict__ rwi,
                                                 const uint32_t* __restrict__ part_w, uint32_t* __restrict__ d_len, unsigned long long* __restrict__ d_rec_off, uint32_t* __restrict__ d_words) {
  const int lane = lane_id();
  const uint32_t n_chunks = (n_rec + 63u) >> 6, n_waves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t chunk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); chunk < n_chunks; chunk += n_waves) {
    const uint32_t i = chunk * 64u + (uint32_t)lane;
    uint32_t len = 0, ro = 0;
    if (i < n_rec) {
      len = rlen[i]; ro = part_w[i / FX_LBLOCK] + rwi[i];
      d_len[i] = len; d_rec_off[(size_t)i + 1u] = (unsigned long long)ro + fx_words(len);
      if (i == 0u) d_rec_off[0] = 0ull;
    }
    const uint32_t units = (len + 31u) >> 5;
    const uint32_t incl = wave_scan_add(units), T = (uint32_t)__shfl((int)incl, 63);
    for (uint32_t base = 0; base < T; base += 64u) {
      const uint32_t t = base + (uint32_t)lane;
      uint32_t src = 0;                                           // the lanes whose units end at or before t: the record of unit t
      for (uint32_t step = 32u; step; step >>= 1) { const uint32_t v = (uint32_t)__shfl((int)incl, (int)min(src + step - 1u, 63u)); if (v <= t) src += step; }
      src = min(src, 63u);
      const uint32_t r_incl = (uint32_t)__shfl((int)incl, (int)src), r_units = (uint32_t)__shfl((int)units, (int)src);
      const uint32_t r_len = (uint32_t)__shfl((int)len, (int)src), r_ro = (uint32_t)__shfl((int)ro, (int)src);
      if (t >= T) continue;
      const uint32_t rec = chunk * 64u + src, k = t - (r_incl - r_units);          // unit k of record rec
      const uint32_t want = min(32u, r_len - 32u * k), cw = (r_len + 15u) >> 4;
      uint32_t j = hdr_line[rec] + 1u, off = 32u * k;
      if (lcum[j + 1u] - lcum[j] != r_len) {                      // the record has several lines: the one that holds letter 32k
        const uint32_t g0 = rcum[rec] + 32u * k;
        uint32_t hi = hdr_line[rec + 1u];
        while (hi - j > 1u) { const uint32_t mid = j + (hi - j) / 2u; if (lcum[mid] <= g0) j = mid; else hi = mid; }
        off = g0 - lcum[j];
      }
      unsigned long long code = 0ull; uint32_t amb = 0u;
      uint32_t s = line_start[j] + off, avail = lcum[j + 1u] - lcum[j] - off;
      if (avail >= want) {
        // one piece: aligned dwords, shifted by the byte phase of s
        const uint32_t a = s & 3u, nd = (a + want + 3u) >> 2;
        const uint32_t* const p32 = reinterpret_cast<const uint32_t*>(text + (s - a));
        uint32_t w[9];
#pragma unroll
        for (uint32_t q = 0; q < 9u; q++) w[q] = q < nd ? p32[q] : 0u;
#pragma unroll
        for (uint32_t q = 0; q < 8u; q++) {
          const uint32_t d = a ? (w[q] >> (8u * a)) | (w[q + 1u] << (32u - 8u * a)) : w[q];
#pragma unroll
          for (uint32_t b = 0; b < 4u; b++) {
            const uint32_t pos = 4u * q + b, c = pos < want ? fx_code((d >> (8u * b)) & 0xFFu) : 0u;
            code |= (unsigned long long)(c & 3u) << (2u * pos); amb |= (c >> 2) << pos;
          }
        }
      } else {
        for (uint32_t got = 0; got < want;) {
          const uint32_t take = min(avail, want - got);
          for (uint32_t q = 0; q < take; q++) { const uint32_t c = fx_code(text[s + q]); code |= (unsigned long long)(c & 3u) << (2u * (got + q)); amb |= (c >> 2) << (got + q); }
          got += take;
          if (got < want) { j++; s = line_start[j]; avail = lcum[j + 1u] - lcum[j]; }
        }
      }
      uint32_t* const cp = d_words + r_ro;
      cp[2u * k] = (uint32_t)code;
      if (2u * k + 1u < cw) cp[2u * k + 1u] = (uint32_t)(code >> 32);
      cp[cw + k] = amb;
    }
  }
}

}  // namespace smr
