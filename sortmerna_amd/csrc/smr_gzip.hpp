// smr_gzip.hpp -- a DEFLATE compressor on the device: byte ranges of one device buffer, cut into chunks of GZ_CHUNK plain bytes, every chunk a
// complete gzip member (RFC 1952: 10-byte header with mtime 0 and no name, the DEFLATE data, CRC-32, ISIZE).  No back-reference crosses a
// chunk, so the members of a stream, laid back to back, are a valid multi-member gzip file -- the shape the reference's own per-thread outputs
// have once Report::merge has concatenated them.
//
//   k_gz_match    one workgroup per chunk.  LZ77 over windows of GZ_WIN positions, one position per thread: the candidate of a position is the
//                 LAST earlier position with the same hash of four bytes that lies in front of the window (table in LDS, inserted with
//                 atomicMax after the window's lookups: the table does not depend on which lane stores last), or the byte in front of it
//                 (runs).  Which positions begin a token is the set reachable from the window's first free position over next[p] = p + len:
//                 eight rounds of pointer doubling, no lane walks the chunk.  Tokens are compacted with a ballot scan into the chunk's token
//                 array; literal/length and distance frequencies are counted with LDS atomics; the CRC-32 of the chunk is put together from
//                 per-thread table CRCs over slices of GZ_SLICE bytes and the GF(2) operators "append 2^k slices of zeros".
//   k_gz_codes    one wave per chunk.  Length-limited Huffman codes (15 / 15 / 7 bits) for the literal/length, distance and code-length
//                 alphabets: rank sort, two-queue merge, depths by walking up; a code that comes out too long is built again from halved
//                 frequencies.  Leaves the bit-reversed codes, the member's first bits (gzip header, block header, the code lengths) and the
//                 member's size -- coded, or stored when coding does not make it smaller.
//   k_gz_encode   one workgroup per chunk.  Per tile of 256 tokens: bit lengths, a scan, the bits OR-ed into an LDS window, the window's whole
//                 dwords stored coalesced into the chunk's worst-case slot.  A stored member is copied as blocks of at most 65 535 bytes.
//   k_gz_compact  one workgroup per chunk: the member from its slot to its place behind the members in front of it (k_export_scan of the sizes).
//
// Text made of rows can be cut at line ends instead (k_gz_cut_lines): nominal cuts every GZ_LINE_PITCH bytes of a stream, each moved back to
// behind the last '\n' of the GZ_LINE_WIN bytes in front of it.  A chunk then holds at most GZ_LINE_PITCH + GZ_LINE_WIN - 1 bytes, within
// GZ_CHUNK, so the four kernels above take such chunks as they are; every member but a stream's last ends with a line, unless a line is longer
// than the window: that one is cut where the grid falls.
#pragma once

namespace smr {

#define GZ_CHUNK 65536u          // plain bytes per member
#define GZ_WIN 256u              // positions per window = threads of k_gz_match
#define GZ_SLICE 256u            // bytes per CRC slice: GZ_CHUNK / GZ_WIN
#define GZ_HASH_BITS 14u
#define GZ_MAXLEN 258u
#define GZ_MAXDIST 32768u
#define GZ_TOK_STRIDE (GZ_CHUNK + 4u)        // tokens of a chunk: at most one per byte + the end-of-block token
#define GZ_NLIT 286u
#define GZ_NDIST 30u
#define GZ_FREQ_STRIDE 320u      // per chunk: 286 literal/length counts at 0, 30 distance counts at 288
#define GZ_PREFIX_WORDS 80u      // 80 bits of gzip header + 3 + 14 + 19 * 3 + 316 * 7 bits of block header at the most
#define GZ_TOK_EOB 256u
#define GZ_CRC_WORDS (256u + 8u * 32u)       // the byte table, then the eight operators of 32 columns each
#define GZ_LINE_PITCH 49152u     // cuts at line ends: the distance of two nominal cuts
#define GZ_LINE_WIN 16384u       // and how far in front of a nominal cut a line end is looked for; GZ_LINE_PITCH + GZ_LINE_WIN = GZ_CHUNK

struct GzChunk { unsigned long long src; uint32_t len, pad; };      // where the chunk's plain bytes begin in the input buffer
// what k_gz_codes leaves per chunk
struct GzCode {
  uint32_t lit[GZ_NLIT + 2];       // bit-reversed code | length << 16
  uint32_t dist[GZ_NDIST + 2];
  uint32_t prefix[GZ_PREFIX_WORDS];
  uint32_t prefix_bits, stored, size, pad;
};

__host__ __device__ __forceinline__ uint32_t gz_stored_size(uint32_t n) { return 18u + n + 5u * ((n + 65534u) / 65535u); }
__host__ __device__ __forceinline__ uint32_t gz_slot_size(uint32_t n) { return (gz_stored_size(n) + 7u) & ~3u; }

// the length symbol of a match of l + 3 bytes: -> symbol, extra bits and their value
__device__ __forceinline__ uint32_t gz_len_sym(uint32_t l, uint32_t& eb, uint32_t& ev) {
  if (l < 8u) { eb = 0; ev = 0; return 257u + l; }
  if (l == 255u) { eb = 0; ev = 0; return 285u; }
  const uint32_t hb = 31u - (uint32_t)__clz((int)l), e = hb - 2u;
  eb = e; ev = l & ((1u << e) - 1u);
  return 257u + 4u * (e + 1u) + ((l >> e) & 3u);
}
// the distance symbol of distance x + 1
__device__ __forceinline__ uint32_t gz_dist_sym(uint32_t x, uint32_t& eb, uint32_t& ev) {
  if (x < 4u) { eb = 0; ev = 0; return x; }
  const uint32_t hb = 31u - (uint32_t)__clz((int)x), e = hb - 1u;
  eb = e; ev = x & ((1u << e) - 1u);
  return 2u * hb + ((x >> e) & 1u);
}
__device__ __forceinline__ uint32_t gz_lit_extra(uint32_t s) { return (s < 265u || s == 285u) ? 0u : (s - 261u) >> 2; }
__device__ __forceinline__ uint32_t gz_dist_extra(uint32_t s) { return s < 4u ? 0u : (s >> 1) - 1u; }

__device__ __forceinline__ uint32_t gz_load4(const uint8_t* __restrict__ p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
__device__ __forceinline__ uint32_t gz_match_len(const uint8_t* __restrict__ s, uint32_t p, uint32_t c, uint32_t maxl) {
  uint32_t l = 0;
  while (l < maxl && s[c + l] == s[p + l]) l++;
  return l;
}
// y = M x over GF(2): column k of M is m[k]
__device__ __forceinline__ uint32_t gz_gf2_apply(const uint32_t* m, uint32_t x) {
  uint32_t y = 0;
  for (uint32_t k = 0; k < 32u; k++) y ^= ((x >> k) & 1u) ? m[k] : 0u;
  return y;
}

// ---- matching ----------------------------------------------------------------------------------------------------------------------------
// tok: GZ_TOK_STRIDE words per chunk of this launch; freq, ntok, crc: per chunk of this launch
__global__ void __launch_bounds__(GZ_WIN) k_gz_match(const uint8_t* __restrict__ in, const GzChunk* __restrict__ chunks, const uint32_t* __restrict__ crc_tab,
                                                     uint32_t* __restrict__ tok, uint32_t* __restrict__ freq, uint32_t* __restrict__ ntok, uint32_t* __restrict__ crc) {
  __shared__ uint32_t s_tab[1u << GZ_HASH_BITS];
  __shared__ uint32_t s_freq[GZ_FREQ_STRIDE];
  __shared__ uint32_t s_crc[GZ_CRC_WORDS];
  __shared__ uint16_t s_next[2][GZ_WIN];
  __shared__ uint8_t s_mark[GZ_WIN];
  __shared__ uint32_t s_wave[4], s_carry[2], s_x[4];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const GzChunk ck = chunks[blockIdx.x];
  const uint8_t* __restrict__ s = in + ck.src;
  const uint32_t n = ck.len;
  uint32_t* __restrict__ my_tok = tok + (size_t)blockIdx.x * GZ_TOK_STRIDE;
  for (uint32_t i = t; i < (1u << GZ_HASH_BITS); i += GZ_WIN) s_tab[i] = 0u;
  for (uint32_t i = t; i < GZ_FREQ_STRIDE; i += GZ_WIN) s_freq[i] = 0u;
  for (uint32_t i = t; i < GZ_CRC_WORDS; i += GZ_WIN) s_crc[i] = crc_tab[i];
  if (t < 2u) s_carry[t] = 0u;
  __syncthreads();

  // CRC-32: thread t takes the slice that ends (GZ_WIN - 1 - t) slices in front of the chunk's end; the thread that owns byte 0 begins with
  // the initial value, which so passes through the same operators as the bytes
  {
    const uint32_t behind = (GZ_WIN - 1u - t) * GZ_SLICE;
    uint32_t x = 0u;
    if (behind < n) {
      const uint32_t e = n - behind, b = e > GZ_SLICE ? e - GZ_SLICE : 0u;
      if (b == 0u) x = 0xFFFFFFFFu;
      for (uint32_t i = b; i < e; i++) x = s_crc[(x ^ s[i]) & 0xFFu] ^ (x >> 8);
      for (uint32_t k = 0; k < 8u; k++) if (((GZ_WIN - 1u - t) >> k) & 1u) x = gz_gf2_apply(s_crc + 256u + 32u * k, x);
    }
    for (int d = 32; d >= 1; d >>= 1) x ^= __shfl_xor(x, d);
    if (lane == 0u) s_x[wv] = x;
  }
  __syncthreads();
  if (t == 0u) crc[blockIdx.x] = s_x[0] ^ s_x[1] ^ s_x[2] ^ s_x[3] ^ 0xFFFFFFFFu;

  uint32_t n_tok = 0;
  for (uint32_t p0 = 0, w = 0; p0 < n; p0 += GZ_WIN, w++) {
    const uint32_t p = p0 + t;
    const bool valid = p < n, hashed = p + 4u <= n;
    uint32_t len = 0, dist = 0, h = 0;
    if (hashed) {
      const uint32_t maxl = min(GZ_MAXLEN, n - p);
      h = (gz_load4(s + p) * 2654435761u) >> (32u - GZ_HASH_BITS);
      const uint32_t c = s_tab[h];
      if (c) {
        const uint32_t d = p - (c - 1u);
        if (d <= GZ_MAXDIST) {
          const uint32_t l = gz_match_len(s, p, c - 1u, maxl);
          if (l >= 4u && !(l == 4u && d > 8192u)) { len = l; dist = d; }
        }
      }
      if (p > 0u) {
        const uint32_t l = gz_match_len(s, p, p - 1u, maxl);
        if (l >= 4u && l > len) { len = l; dist = 1u; }
      }
    }
    const uint32_t carry_in = s_carry[w & 1u];
    s_next[0][t] = (uint16_t)(valid ? min(t + (len ? len : 1u), GZ_WIN + 300u) : GZ_WIN);
    s_mark[t] = (uint8_t)(t == carry_in);
    __syncthreads();                                   // every lookup of the window lies in front of its inserts
    if (hashed) atomicMax(&s_tab[h], p + 1u);
    // the positions reachable from carry_in over next[]: after round k every one of up to 2^(k+1) - 1 steps is marked
    for (uint32_t k = 0, cur = 0; k < 8u; k++, cur ^= 1u) {
      const uint32_t j = s_next[cur][t];
      if (s_mark[t] && j < GZ_WIN) s_mark[j] = 1u;
      s_next[cur ^ 1u][t] = (uint16_t)(j < GZ_WIN ? s_next[cur][j] : j);
      __syncthreads();
    }
    const bool start = valid && s_mark[t] != 0u;
    // (a match that runs past the window: the next one begins behind it; at most one marked position leaves the window)
    if (carry_in >= GZ_WIN) { if (t == 0u) s_carry[(w + 1u) & 1u] = carry_in - GZ_WIN; }
    else if (start && t + (len ? len : 1u) >= GZ_WIN) s_carry[(w + 1u) & 1u] = t + (len ? len : 1u) - GZ_WIN;
    const unsigned long long bal = __ballot(start);
    if (lane == 0u) s_wave[wv] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t base = n_tok, total = 0;
    for (uint32_t k = 0; k < 4u; k++) { const uint32_t c = s_wave[k]; if (k < wv) base += c; total += c; }
    if (start) {
      const uint32_t at = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
      if (len) {
        uint32_t eb, ev;
        my_tok[at] = 0x80000000u | ((len - 3u) << 15) | (dist - 1u);
        atomicAdd(&s_freq[gz_len_sym(len - 3u, eb, ev)], 1u);
        atomicAdd(&s_freq[288u + gz_dist_sym(dist - 1u, eb, ev)], 1u);
      } else {
        const uint32_t b = s[p];
        my_tok[at] = b;
        atomicAdd(&s_freq[b], 1u);
      }
    }
    n_tok += total;
    __syncthreads();                                   // s_wave and s_mark are rewritten by the next window
  }
  if (t == 0u) { my_tok[n_tok] = GZ_TOK_EOB; ntok[blockIdx.x] = n_tok + 1u; }
  for (uint32_t i = t; i < GZ_FREQ_STRIDE; i += GZ_WIN) freq[(size_t)blockIdx.x * GZ_FREQ_STRIDE + i] = s_freq[i] + (i == GZ_TOK_EOB ? 1u : 0u);
}

// ---- codes -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t gz_wave_max(uint32_t v) { for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor(v, d)); return v; }
__device__ __forceinline__ uint32_t gz_wave_sum(uint32_t v) { for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor(v, d); return v; }

// Huffman code lengths of at most `limit` bits for f[0 .. n) (n <= 286; f is halved in place while the code comes out too long) -> len[0 .. n).
// No used symbol: all lengths 0; one: that symbol gets length 1.  One wave; w, par, leaf: scratch of 2n, 2n and n entries.
__device__ __forceinline__ void gz_huff_lengths(uint32_t* f, uint32_t n, uint32_t limit, uint8_t* len, uint32_t* w, uint16_t* par, uint16_t* leaf) {
  const uint32_t lane = threadIdx.x & 63u;
  for (;;) {
    // rank of every used symbol under (frequency, symbol)
    uint32_t m_part = 0;
    for (uint32_t s = lane; s < n; s += 64u) {
      len[s] = 0;
      const uint32_t fs = f[s];
      if (!fs) continue;
      m_part++;
      uint32_t r = 0;
      for (uint32_t u = 0; u < n; u++) { const uint32_t fu = f[u]; r += (fu && (fu < fs || (fu == fs && u < s))) ? 1u : 0u; }
      leaf[r] = (uint16_t)s; w[r] = fs;
    }
    const uint32_t m = gz_wave_sum(m_part);
    __syncthreads();
    if (m == 0u) return;
    if (m == 1u) { if (lane == 0u) len[leaf[0]] = 1; __syncthreads(); return; }
    if (lane == 0u) {                                  // two queues: the sorted leaves and the nodes in the order they were made
      uint32_t i = 0, j = m, k = m;
      while (k < 2u * m - 1u) {
        uint32_t sum = 0;
        for (int q = 0; q < 2; q++) {
          uint32_t x;
          if (i < m && (j >= k || w[i] <= w[j])) x = i++; else x = j++;
          sum += w[x]; par[x] = (uint16_t)k;
        }
        w[k++] = sum;
      }
    }
    __syncthreads();
    uint32_t deepest = 0;
    for (uint32_t r = lane; r < m; r += 64u) {
      uint32_t d = 0;
      for (uint32_t x = r; x != 2u * m - 2u; x = par[x]) d++;
      len[leaf[r]] = (uint8_t)min(d, 255u);
      deepest = max(deepest, d);
    }
    deepest = gz_wave_max(deepest);
    __syncthreads();
    if (deepest <= limit) return;
    for (uint32_t s = lane; s < n; s += 64u) if (f[s]) f[s] = (f[s] + 1u) >> 1;
    __syncthreads();
  }
}
// canonical codes of len[0 .. n) (RFC 1951, 3.2.2), bit-reversed for a stream that is filled from bit 0: code | length << 16 (lane 0)
// next, cnt: 16 words of LDS each (arrays of the lane's own would be indexed by a length and so live in scratch memory)
__device__ __forceinline__ void gz_canonical(const uint8_t* len, uint32_t n, uint32_t* code, uint32_t* next, uint32_t* cnt) {
  for (int b = 0; b < 16; b++) cnt[b] = 0;
  for (uint32_t s = 0; s < n; s++) cnt[len[s]]++;
  cnt[0] = 0;
  uint32_t c = 0;
  next[0] = 0;
  for (int b = 1; b < 16; b++) { c = (c + cnt[b - 1]) << 1; next[b] = c; }
  for (uint32_t s = 0; s < n; s++) {
    const uint32_t l = len[s];
    code[s] = l ? ((__brev(next[l]++) >> (32u - l)) | (l << 16)) : 0u;
  }
}

__device__ __forceinline__ void gz_put_bits(uint32_t* words, uint32_t at, uint32_t v, uint32_t nb) {      // nb <= 25
  if (!nb) return;
  const uint32_t wi = at >> 5, sh = at & 31u;
  atomicOr(&words[wi], v << sh);
  if (sh + nb > 32u) atomicOr(&words[wi + 1u], v >> (32u - sh));
}

__global__ void __launch_bounds__(64) k_gz_codes(const GzChunk* __restrict__ chunks, const uint32_t* __restrict__ freq, GzCode* __restrict__ codes,
                                                 unsigned long long* __restrict__ sizes) {
  __shared__ uint32_t s_f[GZ_NLIT + 2], s_w[2 * GZ_NLIT], s_code[GZ_NLIT + 2], s_prefix[GZ_PREFIX_WORDS], s_clf[20], s_clcode[20];
  __shared__ uint16_t s_par[2 * GZ_NLIT], s_leaf[GZ_NLIT];
  __shared__ uint8_t s_len[GZ_NLIT + GZ_NDIST + 4], s_cllen[20];
  __shared__ uint32_t s_cnt[32];
  const uint32_t lane = threadIdx.x;
  const uint32_t n_plain = chunks[blockIdx.x].len;
  const uint32_t* __restrict__ fq = freq + (size_t)blockIdx.x * GZ_FREQ_STRIDE;
  GzCode* __restrict__ out = codes + blockIdx.x;
  uint32_t bits = 0;                                   // of the tokens under the codes
  // literal/length
  for (uint32_t s = lane; s < GZ_NLIT; s += 64u) s_f[s] = fq[s];
  __syncthreads();
  gz_huff_lengths(s_f, GZ_NLIT, 15u, s_len, s_w, s_par, s_leaf);
  for (uint32_t s = lane; s < GZ_NLIT; s += 64u) bits += fq[s] * ((uint32_t)s_len[s] + gz_lit_extra(s));
  if (lane == 0u) gz_canonical(s_len, GZ_NLIT, s_code, s_cnt, s_cnt + 16);
  __syncthreads();
  for (uint32_t s = lane; s < GZ_NLIT; s += 64u) out->lit[s] = s_code[s];
  __syncthreads();
  // distance
  uint8_t* dlen = s_len + GZ_NLIT;
  for (uint32_t s = lane; s < GZ_NDIST; s += 64u) s_f[s] = fq[288u + s];
  __syncthreads();
  gz_huff_lengths(s_f, GZ_NDIST, 15u, dlen, s_w, s_par, s_leaf);
  for (uint32_t s = lane; s < GZ_NDIST; s += 64u) bits += fq[288u + s] * ((uint32_t)dlen[s] + gz_dist_extra(s));
  if (lane == 0u) gz_canonical(dlen, GZ_NDIST, s_code, s_cnt, s_cnt + 16);
  __syncthreads();
  for (uint32_t s = lane; s < GZ_NDIST; s += 64u) out->dist[s] = s_code[s];
  bits = gz_wave_sum(bits);
  // how many of either are sent: up to the last used one, at least 257 and 1
  uint32_t hl = 0, hd = 0;
  for (uint32_t s = lane; s < GZ_NLIT; s += 64u) if (s_len[s]) hl = max(hl, s + 1u);
  for (uint32_t s = lane; s < GZ_NDIST; s += 64u) if (dlen[s]) hd = max(hd, s + 1u);
  const uint32_t hlit = max(gz_wave_max(hl), 257u), hdist = max(gz_wave_max(hd), 1u), n_len = hlit + hdist;
  __syncthreads();
  // the code-length code over the lengths as they are sent (no run-length symbols)
  if (lane < 19u) s_clf[lane] = 0u;
  for (uint32_t i = lane; i < GZ_PREFIX_WORDS; i += 64u) s_prefix[i] = 0u;
  __syncthreads();
  for (uint32_t i = lane; i < n_len; i += 64u) atomicAdd(&s_clf[i < hlit ? s_len[i] : dlen[i - hlit]], 1u);
  __syncthreads();
  gz_huff_lengths(s_clf, 19u, 7u, s_cllen, s_w, s_par, s_leaf);
  if (lane == 0u) gz_canonical(s_cllen, 19u, s_clcode, s_cnt, s_cnt + 16);
  __syncthreads();
  // the member's first bits: gzip header, BFINAL = 1, BTYPE = 2, HLIT, HDIST, HCLEN, the code-length code, the lengths
  uint32_t hclen = 4;
  {
    const uint32_t order = lane < 19u ? (lane < 3u ? 16u + lane : lane == 3u ? 0u : (lane & 1u) ? 8u - ((lane - 3u) >> 1) : 8u + ((lane - 4u) >> 1)) : 0u;
    // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
    const unsigned long long used = __ballot(lane < 19u && s_cllen[order] != 0u);
    if (used >> 4) hclen = 64u - (uint32_t)__clzll((long long)used);
    if (lane == 0u) {
      s_prefix[0] = 0x00088B1Fu; s_prefix[1] = 0u; s_prefix[2] = 0xFF00u;      // 1f 8b 08 00 | mtime 0 | xfl 0, os 255 (unknown)
      gz_put_bits(s_prefix, 80u, 1u | (2u << 1), 3u);
      gz_put_bits(s_prefix, 83u, hlit - 257u, 5u);
      gz_put_bits(s_prefix, 88u, hdist - 1u, 5u);
      gz_put_bits(s_prefix, 93u, hclen - 4u, 4u);
    }
    if (lane < hclen) gz_put_bits(s_prefix, 97u + 3u * lane, s_cllen[order], 3u);
  }
  uint32_t pos = 97u + 3u * hclen;
  for (uint32_t b = 0; b < n_len; b += 64u) {
    const uint32_t i = b + lane;
    const uint32_t c = i < n_len ? s_clcode[i < hlit ? s_len[i] : dlen[i - hlit]] : 0u;
    const uint32_t nb = c >> 16;
    const uint32_t incl = wave_scan_add(nb);
    gz_put_bits(s_prefix, pos + incl - nb, c & 0xFFFFu, nb);
    pos += (uint32_t)__shfl(incl, 63);
  }
  __syncthreads();
  for (uint32_t i = lane; i < GZ_PREFIX_WORDS; i += 64u) out->prefix[i] = s_prefix[i];
  if (lane == 0u) {
    const uint32_t coded = (pos + bits + 7u) / 8u + 8u, stored = gz_stored_size(n_plain);
    out->prefix_bits = pos;
    out->stored = coded >= stored ? 1u : 0u;
    out->size = min(coded, stored);
    out->pad = 0u;
    sizes[blockIdx.x] = min(coded, stored);
  }
}

// ---- encoding ----------------------------------------------------------------------------------------------------------------------------
// slots: slot_off[chunk] bytes into `slots` (a multiple of 4), gz_slot_size(len) bytes each
__global__ void __launch_bounds__(256) k_gz_encode(const uint8_t* __restrict__ in, const GzChunk* __restrict__ chunks, const uint32_t* __restrict__ tok,
                                                   const uint32_t* __restrict__ ntok, const uint32_t* __restrict__ crc, const GzCode* __restrict__ codes,
                                                   const unsigned long long* __restrict__ slot_off, uint8_t* __restrict__ slots) {
  __shared__ uint32_t s_lit[GZ_NLIT + 2], s_dist[GZ_NDIST + 2];
  __shared__ uint32_t s_win[256u * 2u + 4u];           // 48 bits per token at the most, and the dword the tile begins in
  __shared__ uint32_t s_wave[4];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const GzChunk ck = chunks[blockIdx.x];
  const GzCode* __restrict__ cd = codes + blockIdx.x;
  uint8_t* __restrict__ dst = slots + slot_off[blockIdx.x];
  uint32_t* __restrict__ dst32 = (uint32_t*)dst;
  const uint32_t n = ck.len, sum = crc[blockIdx.x];
  if (cd->stored) {
    const uint8_t* __restrict__ s = in + ck.src;
    const uint32_t nb = (n + 65534u) / 65535u;
    if (t < 10u) dst[t] = t == 0u ? 0x1Fu : t == 1u ? 0x8Bu : t == 2u ? 8u : t == 9u ? 0xFFu : 0u;
    if (t < nb) {
      const uint32_t bl = min(65535u, n - t * 65535u);
      uint8_t* h = dst + 10u + (size_t)t * 65540u;
      h[0] = t + 1u == nb ? 1u : 0u; h[1] = (uint8_t)bl; h[2] = (uint8_t)(bl >> 8); h[3] = (uint8_t)~bl; h[4] = (uint8_t)(~bl >> 8);
    }
    for (uint32_t i = t; i < n; i += 256u) dst[10u + 5u * (i / 65535u + 1u) + i] = s[i];
    if (t < 8u) dst[10u + 5u * nb + n + t] = (uint8_t)((t < 4u ? sum : n) >> (8u * (t & 3u)));
    return;
  }
  for (uint32_t i = t; i < GZ_NLIT; i += 256u) s_lit[i] = cd->lit[i];
  if (t < GZ_NDIST) s_dist[t] = cd->dist[t];
  __syncthreads();
  uint32_t bitpos = cd->prefix_bits;
  for (uint32_t i = t; i < (bitpos >> 5); i += 256u) dst32[i] = cd->prefix[i];
  uint32_t carry = cd->prefix[bitpos >> 5];            // the bits of the dword that is not full yet
  const uint32_t* __restrict__ my_tok = tok + (size_t)blockIdx.x * GZ_TOK_STRIDE;
  const uint32_t n_tok = ntok[blockIdx.x];
  for (uint32_t b = 0; b < n_tok; b += 256u) {
    for (uint32_t i = t; i < 256u * 2u + 4u; i += 256u) s_win[i] = i == 0u ? carry : 0u;
    unsigned long long v = 0;
    uint32_t nb = 0;
    if (b + t < n_tok) {
      const uint32_t k = my_tok[b + t];
      if (k & 0x80000000u) {
        uint32_t eb, ev;
        const uint32_t lc = s_lit[gz_len_sym((k >> 15) & 0xFFu, eb, ev)];
        v = lc & 0xFFFFu; nb = lc >> 16;
        v |= (unsigned long long)ev << nb; nb += eb;
        const uint32_t dc = s_dist[gz_dist_sym(k & 0x7FFFu, eb, ev)];
        v |= (unsigned long long)(dc & 0xFFFFu) << nb; nb += dc >> 16;
        v |= (unsigned long long)ev << nb; nb += eb;
      } else { const uint32_t lc = s_lit[k]; v = lc & 0xFFFFu; nb = lc >> 16; }
    }
    const uint32_t incl = wave_scan_add(nb);
    if (lane == 63u) s_wave[wv] = incl;
    __syncthreads();
    uint32_t at = (bitpos & 31u) + incl - nb, total = 0;
    for (uint32_t k = 0; k < 4u; k++) { const uint32_t c = s_wave[k]; if (k < wv) at += c; total += c; }
    if (nb) {
      const uint32_t wi = at >> 5, sh = at & 31u;
      atomicOr(&s_win[wi], (uint32_t)(v << sh));
      if (sh + nb > 32u) atomicOr(&s_win[wi + 1u], (uint32_t)(v >> (32u - sh)));
      if (sh + nb > 64u) atomicOr(&s_win[wi + 2u], (uint32_t)(v >> (64u - sh)));
    }
    __syncthreads();
    const uint32_t w0 = bitpos >> 5, w1 = (bitpos + total) >> 5;
    for (uint32_t i = t; i < w1 - w0; i += 256u) dst32[w0 + i] = s_win[i];
    carry = s_win[w1 - w0];
    bitpos += total;
    __syncthreads();
  }
  if (t == 0u) {                                       // the bytes of the last dword, then CRC-32 and ISIZE
    uint32_t at = (bitpos >> 5) * 4u;
    const uint32_t end = (bitpos + 7u) >> 3;
    for (uint32_t k = 0; at < end; k++) dst[at++] = (uint8_t)(carry >> (8u * k));
    for (uint32_t k = 0; k < 4u; k++) dst[at++] = (uint8_t)(sum >> (8u * k));
    for (uint32_t k = 0; k < 4u; k++) dst[at++] = (uint8_t)(n >> (8u * k));
  }
}

// ---- compaction ----------------------------------------------------------------------------------------------------------------------------
// the member of every chunk from its slot to out + excl[chunk]; a dword of `out` is stored whole only where all four bytes are the member's
__global__ void __launch_bounds__(256) k_gz_compact(const GzCode* __restrict__ codes, const unsigned long long* __restrict__ slot_off, const uint8_t* __restrict__ slots,
                                                    const unsigned long long* __restrict__ excl, uint8_t* __restrict__ out) {
  const uint32_t t = threadIdx.x;
  const uint32_t size = codes[blockIdx.x].size;
  const uint8_t* __restrict__ src = slots + slot_off[blockIdx.x];
  const uint32_t* __restrict__ src32 = (const uint32_t*)src;
  uint8_t* __restrict__ dst = out + excl[blockIdx.x];
  const uint32_t head = min(size, (uint32_t)((4u - ((uintptr_t)dst & 3u)) & 3u));
  if (t < head) dst[t] = src[t];
  const uint32_t n_dw = (size - head) >> 2;
  uint32_t* __restrict__ dst32 = (uint32_t*)(dst + head);
  // (src + head is `head` bytes behind a dword of the slot; the slot has four spare bytes, so the second dword read is inside it)
  for (uint32_t i = t; i < n_dw; i += 256u) {
    const uint32_t lo = src32[i], hi = src32[i + 1u];
    dst32[i] = head ? (lo >> (8u * head)) | (hi << (32u - 8u * head)) : lo;
  }
  const uint32_t done = head + 4u * n_dw;
  if (t < size - done) dst[done + t] = src[done + t];
}

// ---- cuts at line ends -------------------------------------------------------------------------------------------------------------------
// the place behind the last '\n' of in[b - GZ_LINE_WIN .. b), or b where the window holds none.  The whole workgroup of 256 threads; every
// thread gets the value.  Whole dwords of the window are loaded as dwords, the up to two dwords it shares with its neighbours byte by byte
__device__ __forceinline__ unsigned long long gz_cut_at(const uint8_t* __restrict__ in, unsigned long long b, uint32_t* s_wave) {
  const uint32_t t = threadIdx.x;
  const uintptr_t lo = (uintptr_t)in + (uintptr_t)(b - GZ_LINE_WIN), hi = (uintptr_t)in + (uintptr_t)b;
  uint32_t best = 0;                                   // 1 + the line end's place in the window
  for (uintptr_t w = (lo & ~(uintptr_t)3u) + 4u * t; w < hi; w += 4u * 256u) {
    uint32_t v = 0;
    if (w >= lo && w + 4u <= hi) v = *(const uint32_t*)w;
    else for (uint32_t k = 0; k < 4u; k++) if (w + k >= lo && w + k < hi) v |= (uint32_t)*(const uint8_t*)(w + k) << (8u * k);
    const uint32_t x = v ^ 0x0A0A0A0Au;                // (a byte outside the window is 0 here: no line end)
    for (uint32_t k = 4u; k-- > 0u;) if (((x >> (8u * k)) & 0xFFu) == 0u) { best = (uint32_t)(w + k - lo) + 1u; break; }
  }
  best = gz_wave_max(best);
  if ((t & 63u) == 0u) s_wave[t >> 6] = best;
  __syncthreads();
  best = max(max(s_wave[0], s_wave[1]), max(s_wave[2], s_wave[3]));
  __syncthreads();                                     // (s_wave is written again by the next call)
  return best ? b - GZ_LINE_WIN + best : b;
}

// One workgroup per chunk of the fixed grid: chunk j of stream k (first[k] <= blockIdx.x < first[k + 1]; a stream of n bytes has
// ceil(n / GZ_LINE_PITCH) chunks) lies between cut j - 1 and cut j of the stream, cut -1 its begin, the last cut its end, and cut j otherwise
// gz_cut_at(off[k] + (j + 1) * GZ_LINE_PITCH).  A cut is a function of the text alone, so the workgroup finds both of its own and no cut
// waits for another.  -> chunks[], and in slot_size[] the bytes of the chunk's worst-case slot (gz_run turns them into offsets)
__global__ void __launch_bounds__(256) k_gz_cut_lines(const uint8_t* __restrict__ in, const unsigned long long* __restrict__ off, const unsigned long long* __restrict__ first,
                                                      uint32_t n_streams, GzChunk* __restrict__ chunks, unsigned long long* __restrict__ slot_size) {
  __shared__ uint32_t s_wave[4];
  const unsigned long long c = blockIdx.x;
  uint32_t k = 0, above = n_streams;                   // first[k] <= c < first[above]; streams without bytes share their first[] with the next one
  while (above - k > 1u) { const uint32_t mid = (k + above) >> 1; if (first[mid] <= c) k = mid; else above = mid; }
  const unsigned long long j = c - first[k], m = first[k + 1u] - first[k];
  const unsigned long long begin = j ? gz_cut_at(in, off[k] + j * GZ_LINE_PITCH, s_wave) : off[k];
  const unsigned long long end = j + 1u < m ? gz_cut_at(in, off[k] + (j + 1u) * GZ_LINE_PITCH, s_wave) : off[k + 1u];
  if (threadIdx.x == 0u) {
    GzChunk ck; ck.src = begin; ck.len = (uint32_t)(end - begin); ck.pad = 0u;
    chunks[c] = ck;
    slot_size[c] = gz_slot_size(ck.len);
  }
}

}  // namespace smr
