// smr_fxsplit.hpp -- the aligned.* / other.* FASTX outputs of a batch whose text stayed on the device (SMR_FASTX_KEEP), written there.  The
// definition of every byte is the host writer: smr_reads_record_text (smr_reads.cpp) gives the three strings of a record, write_fx
// (smr_report.cpp) puts them out as  header '\n' letters '\n' [ '+' '\n' quality '\n' ]  and smr_report_add / smr_report_add_pair pick the file.
//
// Logical records.  Layout 0 and 1: record p is read p of the selected batch (layout 1: p and p ^ 1 are mates).  Layout 2: record p is read
// p / 2 of the selected batch (p even) or of the mates' batch (p odd).  In every stream the records stand in the order of p.
//   k_fxs_measure  a thread per logical record: the trimmed header length, where the quality line starts and its trimmed length, whether the
//                  letters lie on one line; the stream (0..3 aligned, 4..7 other, FXS_NONE) from the hit bits of the record and its mate; the
//                  output size.  The text is read as aligned dwordx4 / dwords (it is padded with '\n', so looking for a line's end needs no
//                  bound but the padding).  Then the sizes are summed per stream inside the block of FXS_BLOCK records: every record gets the
//                  bytes of its stream in front of it in the block, the block's eight sums go to part[block][8].
//   k_fxs_scan     one block: part[.][k] to its exclusive sums for the eight streams, the streams' starts to tot[0..8] (tot[8] = all bytes).
//                  All offsets are 64 bit.
//   k_fxs_copy     a wave takes four consecutive records.  When all four are short and have their letters on one line, each gets a team of 16
//                  lanes, else the whole wave takes them one after the other and walks the sequence lines.  A record is a chain of pieces
//                  (text ranges and the literal '\n' / "+\n"); the team keeps the output position and the bytes of the dword that is not yet
//                  full -- the same in every lane -- and puts a piece out as: the bytes that fill the open dword, then whole dwords, lane after
//                  lane, each put together from two aligned dwords of the text by a byte funnel (v_perm_b32) and stored once, then the
//                  piece's last bytes into the open dword.  Only the first and the last dword of a record's range can hold bytes of a
//                  neighbouring record of the stream: of such a dword the team stores ITS bytes only, as bytes.  No atomics, no LDS, and
//                  nothing is stored at or behind the end of the last record.
#pragma once

namespace smr {

#define FXS_BLOCK 1024u        // logical records per block of k_fxs_measure
#define FXS_SHORT 1024u        // output bytes up to which a record whose letters lie on one line is copied by 16 lanes
#define FXS_NONE 8u            // no stream: the record is not written
#define FXS_WIDE 16u           // route bit: the whole wave copies the record
#define FXS_WRAPPED 32u        // route bit: the letters lie on several lines

struct FxsSrc {                // a batch with kept text
  const uint8_t* text; uint32_t n;                              // n bytes of text, '\n' from n to the end of the buffer
  const unsigned long long* hoff; const unsigned long long* soff; const uint32_t* len;
  const RState* state;
};
struct FxsOpts { uint32_t layout, fastq, paired_in, paired_out, out2, sout, want_aligned, want_other; };

__device__ __forceinline__ uint32_t fxs_byte(const uint8_t* __restrict__ text, uint32_t p) {
  return (reinterpret_cast<const uint32_t*>(text)[p >> 2] >> (8u * (p & 3u))) & 0xFFu;
}
// the four bytes at p, whatever its phase: two aligned dwords and a byte funnel
__device__ __forceinline__ uint32_t fxs_load4(const uint8_t* __restrict__ text, uint32_t p) {
  const uint32_t* const t32 = reinterpret_cast<const uint32_t*>(text) + (p >> 2);
  return perm_b32(t32[1], t32[0], 0x03020100u + 0x01010101u * (p & 3u));
}
// the first '\n' at or behind p <= n (text[n] is one)
__device__ __forceinline__ uint32_t fxs_find_nl(const uint8_t* __restrict__ text, uint32_t n, uint32_t p) {
  uint32_t skip = p & 15u;
  for (uint32_t base = p & ~15u; base <= n; base += 16u, skip = 0u) {
    const uint4 v = *reinterpret_cast<const uint4*>(text + base);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t m = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint32_t x = w[q] ^ 0x0A0A0A0Au;
      const uint32_t z = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);      // 0x80 in every byte of x that is 0
      m |= ((((z >> 7) * 0x00204081u) >> 21) & 0xFu) << (4 * q);
    }
    m &= ~((1u << skip) - 1u);
    if (m) return min(base + (uint32_t)__ffs((int)m) - 1u, n);
  }
  return n;
}
__device__ __forceinline__ uint32_t fxs_rtrim(const uint8_t* __restrict__ text, uint32_t s, uint32_t e) {
  while (e > s && fx_trimmed((uint8_t)fxs_byte(text, e - 1u))) e--;
  return e;
}
__device__ __forceinline__ bool fxs_hit(const FxsOpts& o, const FxsSrc& a, const FxsSrc& b, const uint8_t* __restrict__ hit, uint32_t n_a, uint32_t p) {
  const bool second = o.layout == 2u && (p & 1u);
  const uint32_t i = o.layout == 2u ? p >> 1 : p;
  if (hit) return hit[second ? n_a + i : i] != 0;
  const RState* const s = (second ? b.state : a.state) + i;
  return s->n_align != 0u && s->is_hit != 0;                    // (a read without alignments has no record: the host writer sees no hit)
}
// smr_report_add (layout 0) / the table of smr_report_add_pair: mate m of a pair with hit bits h (its own) and hm (its mate's)
__device__ __forceinline__ uint32_t fxs_route(const FxsOpts& o, uint32_t m, bool h, bool hm) {
  uint32_t al = FXS_NONE, ot = FXS_NONE;
  if (o.layout == 0u) { if (h) al = 0u; else ot = 0u; }
  else {
    const bool both = h && hm, any = h || hm;
    const uint32_t num_out = (o.out2 && o.sout) ? 4u : (o.out2 || o.sout) ? 2u : 1u;
    if (any) {
      if (num_out == 1u) { if (o.paired_out ? both : (o.paired_in || h)) al = 0u; }
      else if (num_out == 2u && o.out2) { if (o.paired_out ? both : (o.paired_in || h)) al = m; }
      else if (num_out == 2u) { if (both) al = 0u; else if (h) al = 1u; }
      else { if (both) al = m; else if (h) al = m + 2u; }
    }
    if (!both) {
      if (num_out == 1u) { if (o.paired_in ? !any : (o.paired_out || !h)) ot = 0u; }
      else if (num_out == 2u && o.out2) { if (o.paired_in ? !any : (o.paired_out || !h)) ot = m; }
      else if (num_out == 2u) { if (!any) ot = 0u; else if (!h) ot = 1u; }
      else { if (!any) ot = m; else if (!h) ot = m + 2u; }
    }
  }
  // (a record goes to aligned.* or to other.*, never to both: under every valid option set exactly one of the two tables takes it)
  if (al != FXS_NONE) return o.want_aligned ? al : FXS_NONE;
  if (ot != FXS_NONE) return o.want_other ? 4u + ot : FXS_NONE;
  return FXS_NONE;
}

// rec[p] = {trimmed header length, trimmed quality length, offset of the quality line, stream | FXS_WIDE | FXS_WRAPPED}
__global__ void __launch_bounds__(FXS_BLOCK) k_fxs_measure(uint32_t n_log, FxsOpts o, FxsSrc a, FxsSrc b, const uint8_t* __restrict__ hit, uint4* __restrict__ rec,
                                                           unsigned long long* __restrict__ woff, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long s_w[8][16];
  const uint32_t p = blockIdx.x * FXS_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t stream = FXS_NONE;
  unsigned long long size = 0ull;
  if (p < n_log) {
    const bool second = o.layout == 2u && (p & 1u);
    const uint32_t i = o.layout == 2u ? p >> 1 : p;
    const uint8_t* const text = second ? b.text : a.text;
    const uint32_t n = second ? b.n : a.n;
    const uint32_t h0 = (uint32_t)(second ? b.hoff : a.hoff)[i], s0 = (uint32_t)(second ? b.soff : a.soff)[i], len = (second ? b.len : a.len)[i];
    const uint32_t hl = fxs_rtrim(text, h0, fxs_find_nl(text, n, h0)) - h0;
    uint32_t ql = 0, qoff = 0, flags = 0;
    size = (unsigned long long)hl + 1ull + len + 1ull;
    if (o.fastq) {
      const uint32_t plus = min(fxs_find_nl(text, n, s0 + len) + 1u, n);       // behind the sequence line (no '\n' among its letters)
      qoff = min(fxs_find_nl(text, n, plus) + 1u, n);                          // behind the '+' line
      ql = fxs_rtrim(text, qoff, fxs_find_nl(text, n, qoff)) - qoff;
      size += 2ull + ql + 1ull;
    } else if (len) {
      const uint32_t e = fxs_find_nl(text, n, s0);
      if (fxs_rtrim(text, s0, e) - s0 != len) flags = FXS_WRAPPED | FXS_WIDE;
    }
    if (size > FXS_SHORT) flags |= FXS_WIDE;
    const uint32_t n_a = o.layout == 2u ? n_log >> 1 : n_log;                   // reads of the selected batch
    const bool h = fxs_hit(o, a, b, hit, n_a, p);
    const bool hm = o.layout != 0u && fxs_hit(o, a, b, hit, n_a, p ^ 1u);
    stream = fxs_route(o, p & 1u, h, hm);
    if (stream == FXS_NONE) size = 0ull;
    rec[p] = make_uint4(hl, ql, qoff, stream | flags);
  }
  // the bytes of the record's stream in front of it in this block; the block's sums
  unsigned long long mine = 0ull;
#pragma unroll
  for (uint32_t k = 0; k < 8u; k++) {
    const unsigned long long incl = exp_wave_scan(stream == k ? size : 0ull);
    if (lane == 63u) s_w[k][wv] = incl;
    if (stream == k) mine = incl;
  }
  __syncthreads();
  if (p < n_log) {
    unsigned long long before = 0ull;
    if (stream < 8u) for (uint32_t q = 0; q < wv; q++) before += s_w[stream][q];
    woff[p] = before + mine - size;
  }
  if (threadIdx.x < 8u) {
    unsigned long long all = 0ull;
    for (uint32_t q = 0; q < FXS_BLOCK / 64u; q++) all += s_w[threadIdx.x][q];
    part[(size_t)blockIdx.x * 8u + threadIdx.x] = all;
  }
}

// ---- aligned_denovo.* (smr_fastx_denovo): the same measuring, another predicate and another table; k_fxs_scan and k_fxs_copy serve both ----
// is logical record p a de novo read: n_denovo > 0 and the other three counters 0 (is_dn of smr_report.cpp), or what the caller's bytes say
__device__ __forceinline__ bool fxs_dn(const FxsOpts& o, const uint32_t* __restrict__ ic_a, const uint32_t* __restrict__ ic_b, const uint8_t* __restrict__ dn, uint32_t n_a, uint32_t p) {
  const bool second = o.layout == 2u && (p & 1u);
  const uint32_t i = o.layout == 2u ? p >> 1 : p;
  if (dn) return dn[second ? n_a + i : i] != 0;
  const uint32_t* const ic = second ? ic_b : ic_a;
  if (!ic) return false;                                          // (the pass never ran on the batch)
  const uint4 v = *reinterpret_cast<const uint4*>(ic + 4 * (size_t)i);
  return v.w > 0u && v.x == 0u && v.y == 0u && v.z == 0u;
}
// smr_report_add (layout 0) / the aligned_denovo table of smr_report_add_pair (ReportDenovo::append): mate m, d: it is a de novo read, dm: its
// mate is.  Two quirks of the reference under out2 are the table's, not this function's: under paired_out a pair of which one mate only is a
// de novo read writes nothing; otherwise BOTH mates are written, the one that is no de novo read to file 0.
__device__ __forceinline__ uint32_t fxs_route_dn(const FxsOpts& o, uint32_t m, bool d, bool dm) {
  if (o.layout == 0u) return d ? 0u : FXS_NONE;
  if (!d && !dm) return FXS_NONE;
  const bool both = d && dm;
  const uint32_t num_out = (o.out2 && o.sout) ? 4u : (o.out2 || o.sout) ? 2u : 1u;
  if (num_out == 1u) return (o.paired_in || d) ? 0u : FXS_NONE;
  if (num_out == 2u && o.out2) { if (o.paired_out && !both) return FXS_NONE; return (o.paired_in || d) ? m : 0u; }
  if (num_out == 2u) return both ? 0u : d ? 1u : FXS_NONE;
  return both ? m : d ? m + 2u : FXS_NONE;
}

// k_fxs_measure with fxs_dn / fxs_route_dn: rec[], woff[] and part[][8] as there, the streams 0..3 only
__global__ void __launch_bounds__(FXS_BLOCK) k_fxs_dn_measure(uint32_t n_log, FxsOpts o, FxsSrc a, FxsSrc b, const uint32_t* __restrict__ ic_a, const uint32_t* __restrict__ ic_b,
                                                              const uint8_t* __restrict__ dn, uint4* __restrict__ rec, unsigned long long* __restrict__ woff,
                                                              unsigned long long* __restrict__ part) {
  __shared__ unsigned long long s_w[4][16];
  const uint32_t p = blockIdx.x * FXS_BLOCK + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  uint32_t stream = FXS_NONE;
  unsigned long long size = 0ull;
  if (p < n_log) {
    const bool second = o.layout == 2u && (p & 1u);
    const uint32_t i = o.layout == 2u ? p >> 1 : p;
    const uint8_t* const text = second ? b.text : a.text;
    const uint32_t n = second ? b.n : a.n;
    const uint32_t h0 = (uint32_t)(second ? b.hoff : a.hoff)[i], s0 = (uint32_t)(second ? b.soff : a.soff)[i], len = (second ? b.len : a.len)[i];
    const uint32_t n_a = o.layout == 2u ? n_log >> 1 : n_log;                   // reads of the selected batch
    const bool d = fxs_dn(o, ic_a, ic_b, dn, n_a, p);
    const bool dm = o.layout != 0u && fxs_dn(o, ic_a, ic_b, dn, n_a, p ^ 1u);
    stream = fxs_route_dn(o, p & 1u, d, dm);
    uint32_t hl = 0, ql = 0, qoff = 0, flags = 0;
    if (stream != FXS_NONE) {                                                   // (few reads are de novo reads: the others' text is not looked at)
      hl = fxs_rtrim(text, h0, fxs_find_nl(text, n, h0)) - h0;
      size = (unsigned long long)hl + 1ull + len + 1ull;
      if (o.fastq) {
        const uint32_t plus = min(fxs_find_nl(text, n, s0 + len) + 1u, n);
        qoff = min(fxs_find_nl(text, n, plus) + 1u, n);
        ql = fxs_rtrim(text, qoff, fxs_find_nl(text, n, qoff)) - qoff;
        size += 2ull + ql + 1ull;
      } else if (len) {
        const uint32_t e = fxs_find_nl(text, n, s0);
        if (fxs_rtrim(text, s0, e) - s0 != len) flags = FXS_WRAPPED | FXS_WIDE;
      }
      if (size > FXS_SHORT) flags |= FXS_WIDE;
    }
    rec[p] = make_uint4(hl, ql, qoff, stream | flags);
  }
  unsigned long long mine = 0ull;
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++) {
    const unsigned long long incl = exp_wave_scan(stream == k ? size : 0ull);
    if (lane == 63u) s_w[k][wv] = incl;
    if (stream == k) mine = incl;
  }
  __syncthreads();
  if (p < n_log) {
    unsigned long long before = 0ull;
    if (stream < 4u) for (uint32_t q = 0; q < wv; q++) before += s_w[stream][q];
    woff[p] = before + mine - size;
  }
  if (threadIdx.x < 8u) {
    unsigned long long all = 0ull;
    if (threadIdx.x < 4u) for (uint32_t q = 0; q < FXS_BLOCK / 64u; q++) all += s_w[threadIdx.x][q];
    part[(size_t)blockIdx.x * 8u + threadIdx.x] = all;
  }
}

// part[b][k] -> the bytes of stream k in the blocks in front of b; tot[k] = where stream k starts, tot[8] = all bytes
__global__ void __launch_bounds__(FXS_BLOCK) k_fxs_scan(unsigned long long* __restrict__ part, uint32_t np, unsigned long long* __restrict__ tot) {
  __shared__ unsigned long long s_w[16];
  unsigned long long start = 0ull;
  for (uint32_t k = 0; k < 8u; k++) {
    unsigned long long carry = 0ull;
    for (uint32_t o = 0; o < np; o += FXS_BLOCK) {
      const uint32_t q = o + threadIdx.x;
      const unsigned long long v = q < np ? part[(size_t)q * 8u + k] : 0ull;
      unsigned long long total;
      const unsigned long long incl = exp_block_scan(v, s_w, total);
      if (q < np) part[(size_t)q * 8u + k] = carry + incl - v;
      carry += total;
    }
    if (threadIdx.x == 0) tot[k] = start;
    start += carry;
  }
  if (threadIdx.x == 0) tot[8] = start;
}

// what a team knows of the output while it writes a record: the same in every lane
struct FxsOut {
  uint8_t* out;
  unsigned long long first, pos;      // the record's first byte; the next byte to write
  uint32_t open;                      // the bytes [pos & ~3, pos) in their places, 0 above
};
// the dword at b (a multiple of 4) is full: of a dword that begins in front of the record only the record's bytes are stored
__device__ __forceinline__ void fxs_store(const FxsOut& w, unsigned long long b, uint32_t v) {
  if (b >= w.first) reinterpret_cast<uint32_t*>(w.out)[b >> 2] = v;
  else for (uint32_t q = (uint32_t)(w.first - b); q < 4u; q++) w.out[b + q] = (uint8_t)(v >> (8u * q));
}
// appends the low nb <= 4 bytes of v; `writer`: the one lane of the team that stores
__device__ __forceinline__ void fxs_put(FxsOut& w, uint32_t v, uint32_t nb, bool writer) {
  if (nb == 0u) return;
  if (nb < 4u) v &= (1u << (8u * nb)) - 1u;
  const uint32_t ph = (uint32_t)w.pos & 3u;
  w.open |= v << (8u * ph);
  if (ph + nb >= 4u) {
    if (writer) fxs_store(w, w.pos & ~3ull, w.open);
    w.open = ph ? v >> (32u - 8u * ph) : 0u;
  }
  w.pos += nb;
}
// appends text[s, s + L); lane tl of a team of W
__device__ __forceinline__ void fxs_append(FxsOut& w, const uint8_t* __restrict__ text, uint32_t s, uint32_t L, uint32_t tl, uint32_t W) {
  if (L == 0u) return;
  const uint32_t head = min(L, (4u - ((uint32_t)w.pos & 3u)) & 3u);
  if (head) fxs_put(w, fxs_load4(text, s), head, tl == 0u);
  const uint32_t nd = (L - head) >> 2;
  if (nd) {                                                     // (pos is on a dword now and nothing is open)
    uint32_t* const o32 = reinterpret_cast<uint32_t*>(w.out) + (w.pos >> 2);
    for (uint32_t j = tl; j < nd; j += W) o32[j] = fxs_load4(text, s + head + 4u * j);
    w.pos += 4ull * nd;
  }
  const uint32_t tail = L - head - 4u * nd;
  if (tail) fxs_put(w, fxs_load4(text, s + L - tail), tail, tl == 0u);
}

__global__ void __launch_bounds__(256) k_fxs_copy(uint32_t n_log, FxsOpts o, FxsSrc a, FxsSrc b, const uint4* __restrict__ rec, const unsigned long long* __restrict__ woff,
                                                  const unsigned long long* __restrict__ part, const unsigned long long* __restrict__ tot, uint8_t* __restrict__ out) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t n_quads = (n_log + 3u) >> 2, n_waves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t quad = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); quad < n_quads; quad += n_waves) {
    const uint32_t p0 = quad * 4u;
    uint32_t wide = 0;
    for (uint32_t q = 0; q < 4u; q++) if (p0 + q < n_log) wide |= rec[p0 + q].w & FXS_WIDE;
    const uint32_t W = wide ? 64u : 16u, tl = lane & (W - 1u);
    for (uint32_t it = 0; it < (wide ? 4u : 1u); it++) {
      const uint32_t p = wide ? p0 + it : p0 + (lane >> 4);
      if (p >= n_log) continue;
      const uint4 r = rec[p];
      const uint32_t stream = r.w & 15u;
      if (stream >= FXS_NONE) continue;
      const bool second = o.layout == 2u && (p & 1u);
      const uint32_t i = o.layout == 2u ? p >> 1 : p;
      const uint8_t* const text = second ? b.text : a.text;
      const uint32_t n = second ? b.n : a.n;
      const uint32_t h0 = (uint32_t)(second ? b.hoff : a.hoff)[i], s0 = (uint32_t)(second ? b.soff : a.soff)[i], len = (second ? b.len : a.len)[i];
      FxsOut w;
      w.out = out; w.open = 0u;
      w.first = w.pos = tot[stream] + part[(size_t)(p / FXS_BLOCK) * 8u + stream] + woff[p];
      const bool writer = tl == 0u;
      fxs_append(w, text, h0, r.x, tl, W);
      fxs_put(w, '\n', 1u, writer);
      if (!(r.w & FXS_WRAPPED)) fxs_append(w, text, s0, len, tl, W);
      else {
        for (uint32_t at = s0, done = 0; done < len && at <= n;) {             // the lines of smr_reads_record_text
          const uint32_t e = fxs_find_nl(text, n, at), le = fxs_rtrim(text, at, e);
          fxs_append(w, text, at, le - at, tl, W);
          done += le - at; at = e + 1u;
        }
      }
      fxs_put(w, '\n', 1u, writer);
      if (o.fastq) {
        fxs_put(w, (uint32_t)'+' | ((uint32_t)'\n' << 8), 2u, writer);
        fxs_append(w, text, r.z, r.y, tl, W);
        fxs_put(w, '\n', 1u, writer);
      }
      // the record's last bytes: the dword they lie in can be the next record's as well
      if (writer) for (unsigned long long q = max(w.pos & ~3ull, w.first); q < w.pos; q++) out[q] = (uint8_t)(w.open >> (8u * (uint32_t)(q & 3ull)));
    }
  }
}

}  // namespace smr
