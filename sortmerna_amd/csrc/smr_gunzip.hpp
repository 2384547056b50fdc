// smr_gunzip.hpp -- a DEFLATE decoder on the device: a gzip file (RFC 1952, any number of members) inflated by many waves at once, in the
// manner of pugz / rapidgzip.  A wave cannot know the 32 KiB in front of the place it starts at, so it decodes to 16-bit SYMBOLS: a literal
// byte, or "byte k of the 32 KiB in front of this task"; the symbols become bytes once the windows are known.
//
//   k_gunz_find      one thread per compressed byte.  Tests its eight bit offsets for the header of a non-final dynamic-Huffman block (rule (R):
//                    BFINAL 0, BTYPE 2, HLIT <= 29, HDIST <= 29, a complete code-length code, code lengths that decode without overrun and
//                    without a leading repeat, a code for symbol 256, a complete literal/length code, a distance code that is complete or one
//                    code of one bit) and the byte itself for a gzip member header (1f 8b 08, reserved flag bits zero).  Nearly every offset
//                    fails within the first 13 bits, which are tested on one 64-bit load per thread.  The code-length code of a survivor lives
//                    in two registers (3 bits per symbol, 8 bits per count): no table, no scratch.  Hits are appended to a list with an atomic
//                    counter; the host sorts the few of them (a hit per 16-30 KB of zlib's output).
//   k_gunz_decode    one wave per task, <0> counts, <1> stores symbols.  The loop is uniform across the wave: every lane reads the same bits and
//                    the same LDS tables, so no lane waits for another; the lanes differ where tables are filled, stored blocks are copied
//                    and matches are copied (symbol j of a match comes from `out - dist + j mod dist`, which lies in front of the match: an
//                    overlapping copy needs no second pass).  Stored, fixed and dynamic blocks, member trailers and the following member
//                    headers (FEXTRA, FNAME, FCOMMENT, FHCRC).  It stops at the first block or member boundary at or behind `stop`, at the
//                    end of the data, or after GUNZ_MAXM member boundaries, and refuses what zlib refuses.
//   k_gunz_window    one workgroup, the tasks in order: the resolved 32 KiB behind task i from its own last symbols and the window in front of it.
//   k_gunz_resolve   one workgroup per unit of at most 64 KiB of one task and one member: symbols -> bytes, and the unit's CRC-32 with the byte
//                    table and the slice operators of smr_gzip.hpp.
// Every dependency between workgroups is a kernel boundary.
#pragma once

namespace smr {

#define GUNZ_WIN 32768u
#define GUNZ_MAXM 4u             // member boundaries one task passes at the most
#define GUNZ_LIT_BITS 10u        // index bits of the literal/length table; longer codes are found by counting (as zlib's puff.c does)
#define GUNZ_DIST_BITS 8u
#define GUNZ_UNIT GZ_CHUNK       // bytes per unit of k_gunz_resolve: GZ_WIN slices of GZ_SLICE bytes

#define GUNZ_KIND_BLOCK 0u       // a task starts / ends at a block header (a bit offset)
#define GUNZ_KIND_MEMBER 1u      // ... at a member header (a byte offset)
#define GUNZ_KIND_END 2u         // ends with the data, behind a trailer

#define GUNZ_ERR_TRUNC 1u        // the data end inside a block, a header or a trailer
#define GUNZ_ERR_BTYPE 2u
#define GUNZ_ERR_STORED 3u       // LEN != ~NLEN
#define GUNZ_ERR_HEADER 4u       // a dynamic block's header zlib refuses
#define GUNZ_ERR_CODE 5u         // an unused code, a length symbol 286 / 287, a distance symbol 30 / 31
#define GUNZ_ERR_DIST 6u         // a reference in front of its member's first byte
#define GUNZ_ERR_MAGIC 7u        // no gzip member header where one must be
#define GUNZ_ERR_CAP 8u          // more output than the counting pass found
#define GUNZ_ERR_LONG 9u         // more than GUNZ_PIECE_BITS of the stream in one task: no work for one wave (the host inflates instead)
#define GUNZ_PIECE_BITS (1ull << 29)      // 64 MiB of compressed bytes

struct GunzTask { unsigned long long start, stop, out_off, out_cap; uint32_t kind, pad; };
// a member boundary a task has passed: the trailer's fields, and the header of the member behind it (0, 0: not read by this task)
struct GunzMem { unsigned long long out_rel, hdr_start, hdr_end; uint32_t crc, isize; };
struct GunzRes {
  unsigned long long end, out_len, hdr_start, hdr_end;      // hdr_*: the header a task of kind MEMBER starts at
  uint32_t end_kind, err, n_mem, maxback;                  // maxback: how far in front of the task its first member's references reach
  uint32_t blocks[3], pad;                                 // stored, fixed, dynamic
  GunzMem mem[GUNZ_MAXM];
};
struct GunzUnit { unsigned long long off; uint32_t len, task; };

// 64 bits of the stream from bit bp on (in32 is padded with 16 zero bytes)
__device__ __forceinline__ unsigned long long gunz_peek(const uint32_t* __restrict__ in32, unsigned long long bp) {
  const unsigned long long w = bp >> 5;
  const uint32_t sh = (uint32_t)bp & 31u;
  const unsigned long long lo = (unsigned long long)in32[w] | ((unsigned long long)in32[w + 1u] << 32);
  return sh ? (lo >> sh) | ((unsigned long long)in32[w + 2u] << (64u - sh)) : lo;
}
// the k-th code-length symbol of a dynamic header: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
__device__ __forceinline__ uint32_t gunz_cl_order(uint32_t k) { return k < 3u ? 16u + k : k == 3u ? 0u : (k & 1u) ? 8u - ((k - 3u) >> 1) : 8u + ((k - 4u) >> 1); }

// ---- candidates --------------------------------------------------------------------------------------------------------------------------
// rule (R) for the block header at `bit`, whose first 17 bits the caller has tested
__device__ __forceinline__ bool gunz_rule(const uint32_t* __restrict__ in32, unsigned long long bit, unsigned long long nbits) {
  unsigned long long v = gunz_peek(in32, bit);
  const uint32_t hlit = ((uint32_t)(v >> 3) & 31u) + 257u, hdist = ((uint32_t)(v >> 8) & 31u) + 1u, hclen = ((uint32_t)(v >> 13) & 15u) + 4u;
  unsigned long long bp = bit + 17u;
  if (bp + 3u * hclen > nbits) return false;
  v = gunz_peek(in32, bp);
  bp += 3u * hclen;
  unsigned long long cl = 0, cnt = 0;                  // 3 bits per symbol: its length; 8 bits per length: how many symbols have it
  uint32_t kraft = 0;
  for (uint32_t k = 0; k < hclen; k++) {
    const uint32_t l = (uint32_t)(v >> (3u * k)) & 7u;
    if (l) { cl |= (unsigned long long)l << (3u * gunz_cl_order(k)); kraft += 128u >> l; cnt += 1ull << (8u * l); }
  }
  if (kraft != 128u) return false;
  const uint32_t total = hlit + hdist;
  uint32_t idx = 0, prev = 0, lit = 0, dist = 0, dist_n = 0;
  bool has256 = false;
  while (idx < total) {
    if (bp + 14u > nbits) return false;
    uint32_t w = (uint32_t)gunz_peek(in32, bp), sym = 0, len = 0;
    int code = 0, first = 0;
    for (uint32_t l = 1; l < 8u; l++) {                // (the code is complete: one of the seven lengths matches)
      code |= (int)((w >> (l - 1u)) & 1u);
      const int c = (int)((cnt >> (8u * l)) & 255u);
      if (code - c < first) {
        int target = code - first;                     // the target-th symbol of length l, in symbol order
        for (uint32_t s = 0; s < 19u; s++) if (((uint32_t)(cl >> (3u * s)) & 7u) == l) { if (target == 0) { sym = s; break; } target--; }
        len = l;
        break;
      }
      first = (first + c) << 1; code <<= 1;
    }
    if (!len) return false;
    bp += len; w >>= len;
    uint32_t rep = 1, val = sym;
    if (sym == 16u) { if (idx == 0u) return false; val = prev; rep = 3u + (w & 3u); bp += 2u; }
    else if (sym == 17u) { val = 0; rep = 3u + (w & 7u); bp += 3u; }
    else if (sym == 18u) { val = 0; rep = 11u + (w & 127u); bp += 7u; }
    if (idx + rep > total) return false;
    if (val) {
      const uint32_t nl = idx < hlit ? min(hlit - idx, rep) : 0u;
      lit += nl * (32768u >> val);
      if (idx <= 256u && 256u < idx + nl) has256 = true;
      dist += (rep - nl) * (32768u >> val); dist_n += rep - nl;
    }
    idx += rep; prev = val;
  }
  return has256 && lit == 32768u && (dist == 32768u || (dist_n == 1u && dist == 16384u));
}

// cand: bit offset * 2 + kind, in no order; *n_cand counts every hit, also those behind cap
__global__ void __launch_bounds__(256) k_gunz_find(const uint32_t* __restrict__ in32, unsigned long long n, unsigned long long* __restrict__ cand, uint32_t cap,
                                                   uint32_t* __restrict__ n_cand) {
  const unsigned long long g = (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (g >= n) return;
  const unsigned long long nbits = n * 8u, v = gunz_peek(in32, g * 8u);
  uint32_t hits = 0;
  if ((v & 0xFFFFFFull) == 0x088B1Full && !((v >> 24) & 0xE0u) && g + 18u <= n) hits |= 256u;
  for (uint32_t k = 0; k < 8u; k++) {
    const uint32_t w = (uint32_t)(v >> k);
    if ((w & 7u) != 4u || ((w >> 3) & 31u) > 29u || ((w >> 8) & 31u) > 29u) continue;
    if (g * 8u + k + 17u <= nbits && gunz_rule(in32, g * 8u + k, nbits)) hits |= 1u << k;
  }
  for (uint32_t k = 0; hits; k++, hits >>= 1) {
    if (!(hits & 1u)) continue;
    const uint32_t at = atomicAdd(n_cand, 1u);
    if (at < cap) cand[at] = k == 8u ? g * 16u + GUNZ_KIND_MEMBER : (g * 8u + k) * 2u + GUNZ_KIND_BLOCK;
  }
}

// ---- decoding ----------------------------------------------------------------------------------------------------------------------------
// Canonical code of len[0 .. n) (one wave): cnt[l] symbols of length l, symbol[] the used symbols by (length, symbol), first[l] / start[l] the
// first code of length l and where its symbols begin in symbol[], tab[bit-reversed code, padded to `fast` bits] = symbol | length << 9 for the
// codes of at most `fast` bits (0: none).  -> 0, or 1 where zlib's inflate_table refuses: an over-subscribed code, or an incomplete one that is
// not a single code of one bit (`codes`: the code-length code, which must be complete)
__device__ __forceinline__ uint32_t gunz_build(const uint8_t* len, uint32_t n, uint16_t* cnt, uint16_t* start, uint16_t* first, uint16_t* symbol, uint16_t* tab,
                                               uint32_t fast, uint32_t* stat, uint32_t lane, bool codes) {
  if (lane == 0u) {
    for (uint32_t l = 0; l < 16u; l++) cnt[l] = 0;
    for (uint32_t s = 0; s < n; s++) cnt[len[s]]++;
    const uint32_t used = n - cnt[0];
    int left = 1;
    uint32_t bad = used == 0u && codes ? 1u : 0u;
    for (uint32_t l = 1; l < 16u && !bad; l++) { left = (left << 1) - (int)cnt[l]; if (left < 0) bad = 1u; }
    if (!bad && left > 0 && used != 0u && (codes || !(used == 1u && cnt[1] == 1u))) bad = 1u;
    uint32_t code = 0, at = 0, prev = 0;
    for (uint32_t l = 1; l < 16u; l++) { code = (code + prev) << 1; first[l] = (uint16_t)code; start[l] = (uint16_t)at; at += cnt[l]; prev = cnt[l]; }
    for (uint32_t s = 0; s < n; s++) { const uint32_t l = len[s]; if (l) symbol[start[l]++] = (uint16_t)s; }
    for (uint32_t l = 1; l < 16u; l++) start[l] -= cnt[l];
    *stat = bad;
  }
  for (uint32_t k = lane; k < (1u << fast); k += 64u) tab[k] = 0;
  __syncthreads();
  if (*stat) return 1u;
  const uint32_t used = n - cnt[0];
  for (uint32_t i = lane; i < used; i += 64u) {
    const uint32_t s = symbol[i], l = len[s];
    if (l > fast) continue;
    const uint32_t code = (uint32_t)first[l] + (i - start[l]), rev = __brev(code) >> (32u - l);
    for (uint32_t k = rev; k < (1u << fast); k += 1u << l) tab[k] = (uint16_t)(s | (l << 9));
  }
  __syncthreads();
  return 0u;
}
// the code at the low end of v, found by counting -> symbol | length << 9, 0: no such code
__device__ __forceinline__ uint32_t gunz_slow(uint32_t v, const uint16_t* cnt, const uint16_t* symbol) {
  int code = 0, first = 0, index = 0;
  for (uint32_t l = 1; l < 16u; l++) {
    code |= (int)((v >> (l - 1u)) & 1u);
    const int c = (int)cnt[l];
    if (code - c < first) return (uint32_t)symbol[index + (code - first)] | (l << 9);
    index += c; first = (first + c) << 1; code <<= 1;
  }
  return 0u;
}
// the member header at byte b -> 0 and the first byte behind it, or an error
__device__ __forceinline__ uint32_t gunz_member_header(const uint8_t* __restrict__ in8, unsigned long long n, unsigned long long b, unsigned long long& end) {
  if (b + 10u > n) return GUNZ_ERR_TRUNC;
  if (in8[b] != 0x1Fu || in8[b + 1u] != 0x8Bu || in8[b + 2u] != 8u || (in8[b + 3u] & 0xE0u)) return GUNZ_ERR_MAGIC;
  const uint32_t flg = in8[b + 3u];
  unsigned long long p = b + 10u;
  if (flg & 4u) { if (p + 2u > n) return GUNZ_ERR_TRUNC; p += 2u + ((uint32_t)in8[p] | ((uint32_t)in8[p + 1u] << 8)); if (p > n) return GUNZ_ERR_TRUNC; }
  for (uint32_t f = 8u; f <= 16u; f <<= 1) if (flg & f) { while (p < n && in8[p]) p++; if (p >= n) return GUNZ_ERR_TRUNC; p++; }
  if (flg & 2u) { p += 2u; if (p > n) return GUNZ_ERR_TRUNC; }
  end = p;
  return 0u;
}

// in32: the n compressed bytes (padded); sym: the symbols of all tasks, a task's at its out_off (WRITE only)
template <int WRITE>
__global__ void __launch_bounds__(64) k_gunz_decode(const uint32_t* __restrict__ in32, unsigned long long n, const GunzTask* __restrict__ tasks, GunzRes* __restrict__ res,
                                                    uint16_t* sym) {
  __shared__ uint8_t s_len[320], s_cl[20];             // literal/length lengths at 0, distance lengths at 288; the code-length code's
  __shared__ uint16_t s_cntl[16], s_cntd[16], s_cntc[16], s_start[16], s_first[16];
  __shared__ uint16_t s_syml[288], s_symd[32], s_symc[20];
  __shared__ uint16_t s_tabl[1u << GUNZ_LIT_BITS], s_tabd[1u << GUNZ_DIST_BITS], s_tabc[128];
  __shared__ uint32_t s_stat;
  const uint32_t lane = threadIdx.x;
  const uint8_t* __restrict__ in8 = (const uint8_t*)in32;
  const GunzTask tk = tasks[blockIdx.x];
  GunzRes* __restrict__ r = res + blockIdx.x;
  uint16_t* my_sym = WRITE ? sym + tk.out_off : nullptr;
  const unsigned long long nbits = n * 8u, lim = min(nbits, tk.start + GUNZ_PIECE_BITS);      // where the symbol loop gives up
  unsigned long long bp = tk.start, out = 0, mstart = 0, hdr_s = 0, hdr_e = 0;
  bool mknown = false, need_hdr = tk.kind == GUNZ_KIND_MEMBER;
  uint32_t err = 0, n_mem = 0, maxback = 0, end_kind = GUNZ_KIND_BLOCK, nb0 = 0, nb1 = 0, nb2 = 0;
  for (;;) {
    if (need_hdr) {
      unsigned long long e = 0;
      if ((err = gunz_member_header(in8, n, bp >> 3, e))) break;
      if (n_mem == 0u) { hdr_s = bp >> 3; hdr_e = e; }
      else if (lane == 0u) { r->mem[n_mem - 1u].hdr_start = bp >> 3; r->mem[n_mem - 1u].hdr_end = e; }
      bp = e * 8u; mknown = true; mstart = out; need_hdr = false;
      if (bp >= tk.stop) { end_kind = GUNZ_KIND_BLOCK; break; }      // (the member's first block is a task of its own)
    }
    if (bp + 3u > nbits) { err = GUNZ_ERR_TRUNC; break; }
    if (bp > lim) { err = GUNZ_ERR_LONG; break; }
    unsigned long long v = gunz_peek(in32, bp);
    const uint32_t bfinal = (uint32_t)v & 1u, btype = (uint32_t)(v >> 1) & 3u;
    bp += 3u;
    if (btype == 3u) { err = GUNZ_ERR_BTYPE; break; }
    if (btype == 0u) {
      bp = (bp + 7u) & ~7ull;
      if (bp + 32u > nbits) { err = GUNZ_ERR_TRUNC; break; }
      v = gunz_peek(in32, bp);
      const uint32_t blen = (uint32_t)v & 0xFFFFu;
      if (blen != (((uint32_t)(v >> 16) & 0xFFFFu) ^ 0xFFFFu)) { err = GUNZ_ERR_STORED; break; }
      bp += 32u;
      if (bp + 8ull * blen > nbits) { err = GUNZ_ERR_TRUNC; break; }
      if (WRITE) {
        if (out + blen > tk.out_cap) { err = GUNZ_ERR_CAP; break; }
        for (uint32_t j = lane; j < blen; j += 64u) my_sym[out + j] = in8[(bp >> 3) + j];
      }
      out += blen; bp += 8ull * blen; nb0++;
    } else {
      if (btype == 1u) {
        for (uint32_t i = lane; i < 320u; i += 64u) s_len[i] = (uint8_t)(i < 144u ? 8u : i < 256u ? 9u : i < 280u ? 7u : i < 288u ? 8u : 5u);
        nb1++;
      } else {
        if (bp + 14u > nbits) { err = GUNZ_ERR_TRUNC; break; }
        v = gunz_peek(in32, bp);
        const uint32_t hlit = ((uint32_t)v & 31u) + 257u, hdist = ((uint32_t)(v >> 5) & 31u) + 1u, hclen = ((uint32_t)(v >> 10) & 15u) + 4u;
        bp += 14u;
        if (hlit > 286u || hdist > 30u) { err = GUNZ_ERR_HEADER; break; }
        if (bp + 3u * hclen > nbits) { err = GUNZ_ERR_TRUNC; break; }
        v = gunz_peek(in32, bp);
        bp += 3u * hclen;
        if (lane < 19u) s_cl[gunz_cl_order(lane)] = (uint8_t)(lane < hclen ? (uint32_t)(v >> (3u * lane)) & 7u : 0u);
        for (uint32_t i = lane; i < 320u; i += 64u) s_len[i] = 0;
        __syncthreads();
        if (gunz_build(s_cl, 19u, s_cntc, s_start, s_first, s_symc, s_tabc, 7u, &s_stat, lane, true)) { err = GUNZ_ERR_HEADER; break; }
        const uint32_t total = hlit + hdist;
        uint32_t idx = 0, prev = 0;
        while (idx < total) {
          if (bp > nbits) { err = GUNZ_ERR_TRUNC; break; }
          uint32_t w = (uint32_t)gunz_peek(in32, bp);
          const uint32_t e = s_tabc[w & 127u];
          if (!e) { err = GUNZ_ERR_HEADER; break; }
          const uint32_t s = e & 511u;
          bp += e >> 9; w >>= e >> 9;
          uint32_t rep = 1, val = s;
          if (s == 16u) { if (idx == 0u) { err = GUNZ_ERR_HEADER; break; } val = prev; rep = 3u + (w & 3u); bp += 2u; }
          else if (s == 17u) { val = 0; rep = 3u + (w & 7u); bp += 3u; }
          else if (s == 18u) { val = 0; rep = 11u + (w & 127u); bp += 7u; }
          if (idx + rep > total) { err = GUNZ_ERR_HEADER; break; }
          for (uint32_t j = lane; j < rep; j += 64u) { const uint32_t i = idx + j; s_len[i < hlit ? i : 288u + (i - hlit)] = (uint8_t)val; }
          idx += rep; prev = val;
        }
        if (err) break;
        if (bp > nbits) { err = GUNZ_ERR_TRUNC; break; }
        nb2++;
      }
      __syncthreads();
      if (s_len[256] == 0u) { err = GUNZ_ERR_HEADER; break; }
      if (gunz_build(s_len, 288u, s_cntl, s_start, s_first, s_syml, s_tabl, GUNZ_LIT_BITS, &s_stat, lane, false)) { err = GUNZ_ERR_HEADER; break; }
      if (gunz_build(s_len + 288u, 32u, s_cntd, s_start, s_first, s_symd, s_tabd, GUNZ_DIST_BITS, &s_stat, lane, false)) { err = GUNZ_ERR_HEADER; break; }
      // ---- the symbols of the block
      for (;;) {
        if (bp > lim) { err = bp > nbits ? GUNZ_ERR_TRUNC : GUNZ_ERR_LONG; break; }
        v = gunz_peek(in32, bp);
        uint32_t e = s_tabl[(uint32_t)v & ((1u << GUNZ_LIT_BITS) - 1u)];
        if (!e && !(e = gunz_slow((uint32_t)v, s_cntl, s_syml))) { err = GUNZ_ERR_CODE; break; }
        const uint32_t s = e & 511u;
        bp += e >> 9; v >>= e >> 9;
        if (s < 256u) {
          if (WRITE) { if (out >= tk.out_cap) { err = GUNZ_ERR_CAP; break; } if (lane == 0u) my_sym[out] = (uint16_t)s; }
          out++;
          continue;
        }
        if (s == 256u) break;
        if (s >= 286u) { err = GUNZ_ERR_CODE; break; }
        const uint32_t li = s - 257u, leb = li < 8u || li == 28u ? 0u : (li - 4u) >> 2;
        const uint32_t mlen = li < 8u ? 3u + li : li == 28u ? 258u : 3u + ((4u + (li & 3u)) << leb) + ((uint32_t)v & ((1u << leb) - 1u));
        bp += leb; v >>= leb;
        e = s_tabd[(uint32_t)v & ((1u << GUNZ_DIST_BITS) - 1u)];
        if (!e && !(e = gunz_slow((uint32_t)v, s_cntd, s_symd))) { err = GUNZ_ERR_CODE; break; }
        const uint32_t d = e & 511u;
        if (d >= 30u) { err = GUNZ_ERR_CODE; break; }
        bp += e >> 9; v >>= e >> 9;
        const uint32_t deb = d < 4u ? 0u : (d >> 1) - 1u;
        const uint32_t dist = d < 4u ? 1u + d : 1u + ((2u + (d & 1u)) << deb) + ((uint32_t)v & ((1u << deb) - 1u));
        bp += deb;
        if (dist > out - mstart) {
          if (mknown) { err = GUNZ_ERR_DIST; break; }
          maxback = max(maxback, dist - (uint32_t)out);      // (mstart = 0 while the member's start is not known)
        }
        if (WRITE) {
          if (out + mlen > tk.out_cap) { err = GUNZ_ERR_CAP; break; }
          // The symbols this wave has stored are read here, by other lanes, through plain global stores and loads.  What makes that
          // sufficient: the workgroup IS this one wave, which issues its memory instructions in order; the fence waits for the stores
          // (vmcnt(0)) before the loads are issued, and the CU's L1 is write-through, so a load behind the fence finds them.  It relies
          // on one wave per workgroup and on workgroup scope being one CU: a wider block would need the last symbols in LDS instead.
          __threadfence_block();
          for (uint32_t j = lane; j < mlen; j += 64u) {
            const long long q = (long long)out - (long long)dist + (long long)(j % dist);
            my_sym[out + j] = q >= 0 ? my_sym[q] : (uint16_t)(0x8000u | (uint32_t)(q + (long long)GUNZ_WIN));
          }
        }
        out += mlen;
      }
      if (err) break;
    }
    if (bfinal) {
      bp = (bp + 7u) & ~7ull;
      if (bp + 64u > nbits) { err = GUNZ_ERR_TRUNC; break; }
      v = gunz_peek(in32, bp);
      if (lane == 0u) { GunzMem m; m.out_rel = out; m.hdr_start = 0; m.hdr_end = 0; m.crc = (uint32_t)v; m.isize = (uint32_t)(v >> 32); r->mem[n_mem] = m; }
      n_mem++;
      bp += 64u;
      if (bp == nbits) { end_kind = GUNZ_KIND_END; break; }
      if (bp >= tk.stop || n_mem == GUNZ_MAXM) { end_kind = GUNZ_KIND_MEMBER; break; }
      need_hdr = true;
    } else if (bp >= tk.stop) { end_kind = GUNZ_KIND_BLOCK; break; }
  }
  if (lane == 0u) {
    r->end = bp; r->out_len = out; r->hdr_start = hdr_s; r->hdr_end = hdr_e;
    r->end_kind = end_kind; r->err = err; r->n_mem = n_mem; r->maxback = maxback;
    r->blocks[0] = nb0; r->blocks[1] = nb1; r->blocks[2] = nb2; r->pad = 0;
  }
}

// ---- windows -----------------------------------------------------------------------------------------------------------------------------
// win: GUNZ_WIN bytes per task, the resolved bytes in front of it (task 0's are given).  A window that reaches across a member's start holds
// bytes no reference can name (k_gunz_decode and the host have refused such a reference), so members need no case of their own.
__global__ void __launch_bounds__(1024) k_gunz_window(const GunzTask* __restrict__ tasks, uint32_t n_tasks, const uint16_t* __restrict__ sym, uint8_t* win) {
  const uint32_t t = threadIdx.x;
  for (uint32_t i = 0; i + 1u < n_tasks; i++) {
    const uint8_t* wi = win + (size_t)i * GUNZ_WIN;
    uint8_t* wo = win + (size_t)(i + 1u) * GUNZ_WIN;
    const unsigned long long len = tasks[i].out_cap;
    const uint32_t keep = len >= GUNZ_WIN ? 0u : GUNZ_WIN - (uint32_t)len;       // bytes of the old window that stay
    const uint16_t* __restrict__ tail = sym + tasks[i].out_off + len - (GUNZ_WIN - keep);
    uint32_t s[GUNZ_WIN / 1024u];
#pragma unroll
    for (uint32_t j = 0; j < GUNZ_WIN / 1024u; j++) { const uint32_t k = t + 1024u * j; s[j] = k < keep ? 0x8000u | (k + (GUNZ_WIN - keep)) : tail[k - keep]; }
#pragma unroll
    for (uint32_t j = 0; j < GUNZ_WIN / 1024u; j++) wo[t + 1024u * j] = s[j] < 256u ? (uint8_t)s[j] : wi[s[j] & 0x7FFFu];
    __syncthreads();
  }
}

// ---- bytes and CRC-32 --------------------------------------------------------------------------------------------------------------------
// unit u: out[off, off + len) = the symbols there, resolved through the window of the unit's task; crc[u] = CRC-32 of those bytes
__global__ void __launch_bounds__(GZ_WIN) k_gunz_resolve(const GunzUnit* __restrict__ units, const uint16_t* __restrict__ sym, const uint8_t* __restrict__ win,
                                                        const uint32_t* __restrict__ crc_tab, uint8_t* out, uint32_t* __restrict__ crc) {
  __shared__ uint32_t s_crc[GZ_CRC_WORDS];
  __shared__ uint32_t s_x[4];
  const uint32_t t = threadIdx.x, lane = t & 63u, wv = t >> 6;
  const GunzUnit u = units[blockIdx.x];
  const uint16_t* __restrict__ s = sym + u.off;
  const uint8_t* __restrict__ w = win + (size_t)u.task * GUNZ_WIN;
  uint8_t* o = out + u.off;
  const uint32_t n = u.len;
  for (uint32_t i = t; i < GZ_CRC_WORDS; i += GZ_WIN) s_crc[i] = crc_tab[i];
  for (uint32_t i = t; i < n; i += GZ_WIN) { const uint32_t y = s[i]; o[i] = y < 256u ? (uint8_t)y : w[y & 0x7FFFu]; }
  __syncthreads();
  // (as in k_gz_match: thread t takes the slice that ends GZ_WIN - 1 - t slices in front of the unit's end)
  const uint32_t behind = (GZ_WIN - 1u - t) * GZ_SLICE;
  uint32_t x = 0u;
  if (behind < n) {
    const uint32_t e = n - behind, b = e > GZ_SLICE ? e - GZ_SLICE : 0u;
    if (b == 0u) x = 0xFFFFFFFFu;
    for (uint32_t i = b; i < e; i++) x = s_crc[(x ^ o[i]) & 0xFFu] ^ (x >> 8);
    for (uint32_t k = 0; k < 8u; k++) if (((GZ_WIN - 1u - t) >> k) & 1u) x = gz_gf2_apply(s_crc + 256u + 32u * k, x);
  }
  for (int d = 32; d >= 1; d >>= 1) x ^= __shfl_xor(x, d);
  if (lane == 0u) s_x[wv] = x;
  __syncthreads();
  if (t == 0u) crc[blockIdx.x] = s_x[0] ^ s_x[1] ^ s_x[2] ^ s_x[3] ^ 0xFFFFFFFFu;
}

}  // namespace smr
