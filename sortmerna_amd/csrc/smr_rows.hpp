// smr_rows.hpp -- the rows of aligned.sam and of the BLAST tabular report for the stored alignments of one (index, part), written on the
// device from what is in HBM after smr_traceback: the kept FASTX text (SMR_FASTX_KEEP), the packed letters and ambiguity masks, AlignRec and
// the CIGAR pool, the part's reference letters.  The definition of every byte is add_rows / cigar_text of smr_report.cpp.
//
//   k_rows_stat   16 lanes per alignment slot, four slots per wave: n_miss / n_gap / n_match of Read::calc_miss_gap_match along the CIGAR over
//                 the STRAND-CORRECT read letters (the reverse complement for strand 0: the writers call revIntStr, unlike the %id / %coverage
//                 pass of smr_idcov.hpp) and the reference letters; and everything the host writer would read out of bounds for: a CIGAR
//                 that is missing, has no columns or runs past its read or reference, a ref_num beyond the part.  Nothing is written for a
//                 batch with such an alignment (err[] counts them).  The only atomics of the family are these error counts.
//   k_rows_size   a thread per read: where its id and its quality line lie in the text (meta[]), the bytes of its rows in each stream, summed
//                 inside the block (exp_block_scan); k_export_scan turns the blocks' sums into their exclusive sums.  64-bit offsets.
//   k_rows_write  a wave takes 64 consecutive reads, whose rows are one contiguous byte range of a stream, and puts them together piece by
//                 piece in a window of LDS that starts on a dword of the output: every lane a byte of a piece at a time (text, the letters of
//                 SEQ, a number's digits), the operations of a CIGAR 64 at a time with their places from wave_scan_add.  The window's whole
//                 dwords are stored lane after lane (exp_flush of smr_export.hpp); the first and the last dword of the wave's range, which
//                 neighbouring waves share, are stored as bytes.  A row longer than the window (a 5 kb read) streams through it.  No atomics.
// Both kernels run the same row functions (rows_sam, rows_blast) over a sink: RowsCount adds lengths, RowsWave writes -- a row has one
// definition here.
//
// Numbers.  %id and qcov are `%.3g` of a binary double: rows_fmt takes the double's mantissa and exponent and finds the three digits by
// exact integer arithmetic (128-bit), rounding to nearest-even on the exact value like glibc.  E-value and bit score depend on the database
// and score1 only: their texts come from a table the host made with the host writer's own function (smr::score_texts).
#pragma once

namespace smr {

#define ROWS_WINDOW 4096u       // bytes of LDS window per wave of k_rows_write
#define ROWS_BLOCK 256u         // reads per block of k_rows_size
#define ROWS_TAB_ENTRY 32u      // bytes per score of the e-value / bit-score table: two lengths, 14 bytes of e-value, 16 of bit score
enum { ROWS_E_NOCIG = 1, ROWS_E_NOCOLS, ROWS_E_PAST, ROWS_E_BADREF, ROWS_E_SCORE, ROWS_E_COUNT };
enum { ROWS_COL_CIGAR = 1, ROWS_COL_QCOV, ROWS_COL_QSTRAND };

struct RowsSrc { const uint8_t* text; uint32_t n_text, fastq; const unsigned long long* hoff; const unsigned long long* soff; };
struct RowsRef { const uint8_t* names; const uint32_t* name_off; const uint8_t* tab; };
#define ROWS_MAX_COLS 12u
struct RowsOpts { uint32_t want_sam, want_blast, ncols, cols, index_num, part, n_tab; };      // cols: two bits per optional column (ROWS_COL_*), the first lowest

// up to 16 characters in two registers (an array indexed by the lane would live in scratch)
struct RowsStr { unsigned long long lo, hi; uint32_t len; };
__device__ __forceinline__ void rows_push(RowsStr& s, uint32_t ch) {
  if (s.len < 8u) s.lo |= (unsigned long long)ch << (8u * s.len);
  else if (s.len < 16u) s.hi |= (unsigned long long)ch << (8u * (s.len - 8u));
  s.len++;
}
__device__ __forceinline__ uint8_t rows_char(const RowsStr& s, uint32_t j) { return (uint8_t)(j < 8u ? s.lo >> (8u * j) : s.hi >> (8u * (j - 8u))); }
// |v| < 10^15, which is what 32-bit fields and their sums give
__device__ __forceinline__ RowsStr rows_num(long long v) {
  unsigned long long u = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
  unsigned __int128 acc = 0;
  uint32_t nd = 0;
  do { acc = (acc << 8) | (unsigned)('0' + (unsigned)(u % 10ull)); u /= 10ull; nd++; } while (u && nd < 15u);
  if (v < 0) { acc = (acc << 8) | (unsigned)'-'; nd++; }
  RowsStr s; s.lo = (unsigned long long)acc; s.hi = (unsigned long long)(acc >> 64); s.len = nd;
  return s;
}
__device__ __forceinline__ uint32_t rows_digits(uint32_t v) {
  uint32_t d = 1;
  for (uint32_t p = 10u; d < 10u && v >= p; p *= 10u) d++;       // (d == 10: p would wrap)
  return d;
}
template <unsigned N> __device__ __forceinline__ constexpr unsigned long long rows_pack(const char (&s)[N]) {
  static_assert(N <= 9, "rows_pack: at most eight characters");
  unsigned long long v = 0;
  for (unsigned i = 0; i + 1 < N; i++) v |= (unsigned long long)(unsigned char)s[i] << (8u * i);
  return v;
}
#define ROWS_LIT(sink, text) (sink).lit(rows_pack(text), (uint32_t)sizeof(text) - 1u)

// `%.3g` of (double)num / (double)den * 100 for den > 0: the text of `stream << x` at precision 3.  The double is the host's (an IEEE
// division and a product, each rounded once: contraction off); the decimal digits come from its exact value m * 2^e.  With 32-bit num and
// den a non-zero x lies in [2.3e-8, 4.3e11]: e < 0, and every product below stays under 2^100.
__device__ __forceinline__ RowsStr rows_fmt(uint32_t num, uint32_t den) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  RowsStr s; s.lo = 0; s.hi = 0; s.len = 0;
  const double ratio = (double)num / (double)den;
  const double x = ratio * 100.0;
  unsigned long long bits;
  __builtin_memcpy(&bits, &x, 8);
  if ((bits << 1) == 0ull) { rows_push(s, '0'); return s; }
  const int e = (int)((bits >> 52) & 0x7FFull) - 1075;
  const unsigned long long m = (bits & ((1ull << 52) - 1ull)) | (1ull << 52);
  int X = ((e + 52) * 1233) >> 12;                    // floor(log10 x), at most one off
  unsigned q = 0;
  unsigned __int128 N = 0, D = 1;
  for (int it = 0; it < 4; it++) {                    // x / 10^(X - 2) = N / D, q = its integer part: 100 .. 999 when X is right
    const int k = X - 2, ak = k < 0 ? -k : k;
    N = m; D = 1;
    if (e >= 0) N <<= e; else D <<= -e;
    unsigned long long p10 = 1ull;
    for (int j = 0; j < ak && j < 19; j++) p10 *= 10ull;
    if (k < 0) N *= p10; else D *= p10;
    q = 0;
    for (int bit = 13; bit >= 0; bit--) { const unsigned t = q | (1u << bit); if (D * t <= N) q = t; }
    if (q >= 1000u) X++; else if (q < 100u) X--; else break;
  }
  const unsigned __int128 twice = (N - D * q) << 1;   // round to nearest, ties to even, on the exact value
  if (twice > D || (twice == D && (q & 1u))) q++;
  if (q >= 1000u) { q = 100u; X++; }
  const uint32_t d[3] = {q / 100u, (q / 10u) % 10u, q % 10u};
  const uint32_t sig = d[2] ? 3u : d[1] ? 2u : 1u;     // %g drops trailing zeros
  if (X < -4 || X >= 3) {
    rows_push(s, '0' + d[0]);
    if (sig > 1u) { rows_push(s, '.'); rows_push(s, '0' + d[1]); if (sig > 2u) rows_push(s, '0' + d[2]); }
    rows_push(s, 'e'); rows_push(s, X < 0 ? '-' : '+');
    const uint32_t ax = (uint32_t)(X < 0 ? -X : X);
    if (ax >= 100u) rows_push(s, '0' + ax / 100u);
    rows_push(s, '0' + (ax / 10u) % 10u); rows_push(s, '0' + ax % 10u);
  } else if (X >= 0) {
    rows_push(s, '0' + d[0]);
    if (X >= 1 || sig > 1u) { if (X == 0) rows_push(s, '.'); rows_push(s, '0' + d[1]); }      // (the point stands behind digit X)
    if (X >= 2 || sig > 2u) { if (X == 1) rows_push(s, '.'); rows_push(s, '0' + d[2]); }
  } else {
    rows_push(s, '0'); rows_push(s, '.');
    for (int z = 0; z < -X - 1; z++) rows_push(s, '0');
    rows_push(s, '0' + d[0]);
    if (sig > 1u) rows_push(s, '0' + d[1]);
    if (sig > 2u) rows_push(s, '0' + d[2]);
  }
  return s;
}

// letter p (0..4) of the read as the report writers walk it: the forward letters for strand 1, the reverse complement for strand 0
__device__ __forceinline__ uint32_t rows_letter(const uint32_t* __restrict__ rec, uint32_t cw, uint32_t readlen, uint32_t strand, uint32_t p) {
  const uint32_t q = strand ? p : readlen - 1u - p;
  const uint32_t code = (rec[q >> 4] >> ((q & 15u) * 2u)) & 3u;
  if ((rec[cw + (q >> 5)] >> (q & 31u)) & 1u) return 4u;
  return strand ? code : 3u - code;
}
__device__ __forceinline__ bool rows_mine(const AlignRec& a, const RowsOpts& o) { return a.index_num == o.index_num && a.part == o.part; }

// ---- the two sinks -------------------------------------------------------------------------------------------------------------------
struct RowsCount {
  unsigned long long n;
  __device__ __forceinline__ void str(const RowsStr& s) { n += s.len; }
  __device__ __forceinline__ void lit(unsigned long long, uint32_t len) { n += len; }
  __device__ __forceinline__ void text(const uint8_t*, uint32_t, uint32_t len, bool) { n += len; }
  __device__ __forceinline__ void seq(const uint32_t*, uint32_t, uint32_t readlen, uint32_t) { n += readlen; }
  __device__ __forceinline__ void ops(const uint32_t* __restrict__ cigar, unsigned long long pool_words, uint32_t off, uint32_t cnt) {
    for (uint32_t q = 0; q < cnt; q++) n += rows_digits(exp_cigar_word(cigar, pool_words, (unsigned long long)off + q) >> 4) + 1u;
  }
};
// the wave's window: holds the output bytes [wbase, pos), wbase on a dword; every member is called by the whole wave with equal arguments
struct RowsWave {
  uint32_t* win; uint8_t* win8; uint8_t* out;
  unsigned long long wbase, pos, first;
  int lane;
  __device__ __forceinline__ void flush() { exp_flush(win, out, wbase, pos, first, lane); }
  __device__ __forceinline__ void room(uint32_t len) { if (pos - wbase + len > ROWS_WINDOW) flush(); }
  __device__ __forceinline__ void str(const RowsStr& s) {
    room(16u);
    if ((uint32_t)lane < s.len) win8[(uint32_t)(pos - wbase) + (uint32_t)lane] = rows_char(s, (uint32_t)lane);
    pos += s.len;
  }
  __device__ __forceinline__ void lit(unsigned long long packed, uint32_t len) {
    room(8u);
    if ((uint32_t)lane < len) win8[(uint32_t)(pos - wbase) + (uint32_t)lane] = (uint8_t)(packed >> (8u * (uint32_t)lane));
    pos += len;
  }
  // len bytes, byte j = f(j); longer than the window's room: in pieces, the window stored in between
  template <class F> __device__ __forceinline__ void run(uint32_t len, F f) {
    for (uint32_t at = 0; at < len;) {
      uint32_t space = ROWS_WINDOW - (uint32_t)(pos - wbase);
      if (space < len - at && space < ROWS_WINDOW / 2u) { flush(); space = ROWS_WINDOW - (uint32_t)(pos - wbase); }
      const uint32_t take = min(len - at, space), w0 = (uint32_t)(pos - wbase);
      for (uint32_t j = (uint32_t)lane; j < take; j += 64u) win8[w0 + j] = f(at + j);
      pos += take; at += take;
    }
  }
  __device__ __forceinline__ void text(const uint8_t* __restrict__ base, uint32_t off, uint32_t len, bool reversed) {
    run(len, [&](uint32_t j) { return (uint8_t)fxs_byte(base, off + (reversed ? len - 1u - j : j)); });
  }
  __device__ __forceinline__ void seq(const uint32_t* __restrict__ rec, uint32_t cw, uint32_t readlen, uint32_t strand) {
    run(readlen, [&](uint32_t j) { return (uint8_t)(0x4E54474341ull >> (8u * rows_letter(rec, cw, readlen, strand, j))); });      // "ACGTN"
  }
  __device__ __forceinline__ void ops(const uint32_t* __restrict__ cigar, unsigned long long pool_words, uint32_t off, uint32_t cnt) {
    for (uint32_t q0 = 0; q0 < cnt; q0 += 64u) {
      const uint32_t q = q0 + (uint32_t)lane;
      const uint32_t c = q < cnt ? exp_cigar_word(cigar, pool_words, (unsigned long long)off + q) : 0u;
      RowsStr s = rows_num((long long)(c >> 4));
      rows_push(s, (c & 0xFu) == 0u ? 'M' : ((c & 0xFu) == 1u ? 'I' : 'D'));
      const uint32_t l = q < cnt ? s.len : 0u;
      const uint32_t incl = wave_scan_add(l), tot = (uint32_t)__shfl((int)incl, 63, 64);
      room(tot);                                       // (64 operations of at most 10 characters)
      const uint32_t w0 = (uint32_t)(pos - wbase) + incl - l;
      for (uint32_t j = 0; j < l; j++) win8[w0 + j] = rows_char(s, j);
      pos += tot;
    }
  }
};

// ---- a row, for either sink ------------------------------------------------------------------------------------------------------------
struct RowsRead {               // what the rows of one read share
  const uint32_t* rec; uint32_t cw, readlen;
  uint32_t id_off, id_len, q_off, q_len;
};
template <class S> __device__ __forceinline__ void rows_cigar(S& s, const AlignRec& a, const RowsRead& R, const uint32_t* __restrict__ cigar, unsigned long long pool_words) {
  if (a.read_begin1 != 0) { RowsStr t = rows_num((long long)a.read_begin1); rows_push(t, 'S'); s.str(t); }
  s.ops(cigar, pool_words, a.cigar_off, a.cigar_len);
  const long long end_mask = (long long)R.readlen - (long long)a.read_end1 - 1ll;
  if (end_mask > 0) { RowsStr t = rows_num(end_mask); rows_push(t, 'S'); s.str(t); }
}
__device__ __forceinline__ void rows_ref_name(const RowsRef& ref, uint32_t ref_num, uint32_t& off, uint32_t& len) {
  off = ref.name_off[ref_num]; len = ref.name_off[ref_num + 1u] - off;
}
// q_reversed: the quality line as the writer's copy of it stands at this alignment (reversed in place at every strand-0 alignment of the key)
template <class S> __device__ __forceinline__ void rows_sam(S& s, const AlignRec& a, const uint4& st, const RowsRead& R, const RowsSrc& src, const RowsRef& ref,
                                                            const uint32_t* __restrict__ cigar, unsigned long long pool_words, bool q_reversed) {
  uint32_t no, nl;
  rows_ref_name(ref, a.ref_num, no, nl);
  s.text(src.text, R.id_off, R.id_len, false);
  if (a.strand) ROWS_LIT(s, "\t0\t"); else ROWS_LIT(s, "\t16\t");
  s.text(ref.names, no, nl, false);
  ROWS_LIT(s, "\t");
  s.str(rows_num((long long)a.ref_begin1 + 1ll));
  ROWS_LIT(s, "\t255\t");
  rows_cigar(s, a, R, cigar, pool_words);
  ROWS_LIT(s, "\t*\t0\t0\t");
  s.seq(R.rec, R.cw, R.readlen, a.strand);
  ROWS_LIT(s, "\t");
  if (src.fastq && R.q_len) s.text(src.text, R.q_off, R.q_len, q_reversed); else ROWS_LIT(s, "*");
  ROWS_LIT(s, "\tAS:i:");
  s.str(rows_num((long long)a.score1));
  ROWS_LIT(s, "\tNM:i:");
  RowsStr t = rows_num((long long)(uint32_t)(st.x + st.y));
  rows_push(t, '\n');
  s.str(t);
}
template <class S> __device__ __forceinline__ void rows_tab_num(S& s, long long v) { RowsStr t = rows_num(v); rows_push(t, '\t'); s.str(t); }
template <class S> __device__ __forceinline__ void rows_blast(S& s, const AlignRec& a, const uint4& st, const RowsRead& R, const RowsSrc& src, const RowsRef& ref,
                                                              const RowsOpts& o, const uint32_t* __restrict__ cigar, unsigned long long pool_words) {
  uint32_t no, nl;
  rows_ref_name(ref, a.ref_num, no, nl);
  s.text(src.text, R.id_off, R.id_len, false);
  ROWS_LIT(s, "\t");
  s.text(ref.names, no, nl, false);
  ROWS_LIT(s, "\t");
  { RowsStr t = rows_fmt(st.z, st.x + st.y + st.z); rows_push(t, '\t'); s.str(t); }
  const long long span = (long long)(a.read_end1 - a.read_begin1 + 1);
  rows_tab_num(s, span);
  rows_tab_num(s, (long long)st.x);
  rows_tab_num(s, (long long)st.y);
  rows_tab_num(s, (long long)a.read_begin1 + 1ll);
  rows_tab_num(s, (long long)a.read_end1 + 1ll);
  rows_tab_num(s, (long long)a.ref_begin1 + 1ll);
  rows_tab_num(s, (long long)a.ref_end1 + 1ll);
  const uint32_t te = (uint32_t)a.score1 * ROWS_TAB_ENTRY;
  s.text(ref.tab, te + 2u, fxs_byte(ref.tab, te), false);
  ROWS_LIT(s, "\t");
  s.text(ref.tab, te + 16u, fxs_byte(ref.tab, te + 1u), false);
  for (uint32_t k = 0; k < o.ncols; k++) {
    ROWS_LIT(s, "\t");
    const uint32_t col = (o.cols >> (2u * k)) & 3u;
    if (col == ROWS_COL_CIGAR) rows_cigar(s, a, R, cigar, pool_words);
    else if (col == ROWS_COL_QCOV) s.str(rows_fmt((uint32_t)(span < 0 ? -span : span), a.readlen));
    else if (a.strand) ROWS_LIT(s, "+"); else ROWS_LIT(s, "-");
  }
  ROWS_LIT(s, "\n");
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------------------
// stat[i] = {n_miss, n_gap, n_match, what is wrong with it (ROWS_E_*) or 0} for every alignment slot i of the batch that holds an alignment of (index_num, part)
__global__ void __launch_bounds__(256) k_rows_stat(DReads rd, DIndex ix, uint32_t slots, const RState* __restrict__ saved, const AlignRec* __restrict__ aln,
                                                   const uint32_t* __restrict__ cigar, unsigned long long pool_words, RowsOpts o, uint4* __restrict__ stat, uint32_t* __restrict__ err) {
  const uint32_t lane = (uint32_t)lane_id(), g = lane >> 4, gl = lane & 15u;
  const unsigned long long total = (unsigned long long)rd.n * slots, n_waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
  for (unsigned long long base = ((unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 4ull; base < total; base += n_waves * 4ull) {
    const unsigned long long i = base + g;
    bool have = i < total;
    AlignRec a; a.cigar_len = 0; a.cigar_off = 0; a.strand = 1;
    uint32_t r = 0;
    if (have) {
      r = (uint32_t)(i / slots);
      have = (uint32_t)(i - (unsigned long long)r * slots) < min(saved[r].n_align, slots);
      if (have) { a = aln[i]; have = rows_mine(a, o); }
    }
    uint32_t bad = 0;
    if (have) {
      if (!(a.has_cigar & 1u)) bad = ROWS_E_NOCIG;
      else if (a.ref_num >= ix.n_refs) bad = ROWS_E_BADREF;
      else if (a.read_begin1 < 0 || a.ref_begin1 < 0) bad = ROWS_E_PAST;
    }
    const bool walk = have && !bad;
    const uint32_t* rec = rd.words; uint32_t cw = 0, readlen = 0;
    unsigned long long pb = 0, qb = 0, ref_end = 0;
    if (walk) {
      rec = rd.words + rd.rec_off[r]; readlen = rd.len[r]; cw = (readlen + 15u) >> 4;
      pb = (unsigned long long)a.read_begin1; qb = ix.ref_off[a.ref_num] + (unsigned long long)a.ref_begin1; ref_end = ix.ref_off[a.ref_num + 1];
    }
    const uint32_t ncig = walk ? a.cigar_len : 0u;
    uint32_t maxc = ncig;
    for (int d = 32; d >= 16; d >>= 1) maxc = max(maxc, (uint32_t)__shfl_xor((int)maxc, d, 64));
    uint32_t n_match = 0, n_miss = 0, n_gap = 0;
    for (uint32_t q = 0; q < maxc; q++) {
      if (q < ncig) {
        const uint32_t c = exp_cigar_word(cigar, pool_words, (unsigned long long)a.cigar_off + q), op = c & 0xFu, len = c >> 4;
        if (op == 0u) {
          unsigned long long ok = len;                 // columns inside the read and the reference sequence
          ok = pb < readlen ? min(ok, (unsigned long long)readlen - pb) : 0ull;
          ok = qb < ref_end ? min(ok, ref_end - qb) : 0ull;
          for (uint32_t k = gl; k < (uint32_t)ok; k += 16u) {
            if (rows_letter(rec, cw, readlen, a.strand, (uint32_t)pb + k) != (uint32_t)ix.ref_seq[qb + k]) n_miss++; else n_match++;
          }
          if (gl == 0u) n_miss += len - (uint32_t)ok;
          pb += len; qb += len;
        } else { if (op == 1u) pb += len; else qb += len; if (gl == 0u) n_gap += len; }
      }
    }
    for (int d = 8; d > 0; d >>= 1) { n_match += __shfl_xor((int)n_match, d, 64); n_miss += __shfl_xor((int)n_miss, d, 64); n_gap += __shfl_xor((int)n_gap, d, 64); }
    if (have && gl == 0u) {
      if (!bad) {
        if (pb > readlen || qb > ref_end) bad = ROWS_E_PAST;
        else if (n_miss + n_gap + n_match == 0u) bad = ROWS_E_NOCOLS;
        else if (o.want_blast && a.score1 >= o.n_tab) bad = ROWS_E_SCORE;
      }
      if (bad) atomicAdd(&err[bad], 1u);
      stat[i] = make_uint4(n_miss, n_gap, n_match, bad);
    }
  }
}

// excl_*[i]: the bytes of the rows of the block's reads in front of read i, per stream; part_*[b]: block b's bytes (entry np: 0, for the scan
// to leave the total there); meta[i] = {offset and length of the id in the text, offset and trimmed length of the quality line}
__global__ void __launch_bounds__(ROWS_BLOCK) k_rows_size(DReads rd, uint32_t slots, const RState* __restrict__ saved, const AlignRec* __restrict__ aln,
                                                          const uint32_t* __restrict__ cigar, unsigned long long pool_words, const uint4* __restrict__ stat,
                                                          RowsSrc src, RowsRef ref, RowsOpts o, uint4* __restrict__ meta,
                                                          unsigned long long* __restrict__ excl_s, unsigned long long* __restrict__ excl_b,
                                                          unsigned long long* __restrict__ part_s, unsigned long long* __restrict__ part_b) {
  __shared__ unsigned long long s_w[16];
  const uint32_t i = blockIdx.x * ROWS_BLOCK + threadIdx.x;
  RowsCount cs, cb; cs.n = 0; cb.n = 0;
  if (i < rd.n) {
    const uint32_t na = min(saved[i].n_align, slots);
    bool any = false;
    for (uint32_t k = 0; k < na; k++) any = any || rows_mine(aln[(size_t)i * slots + k], o);
    if (any) {
      RowsRead R;
      R.readlen = rd.len[i]; R.cw = (R.readlen + 15u) >> 4; R.rec = rd.words + rd.rec_off[i];
      // Read::getSeqId on the trimmed header line: up to the first ' ', without the leading '>' / '@'
      const uint32_t h0 = (uint32_t)src.hoff[i], he = fxs_rtrim(src.text, h0, fxs_find_nl(src.text, src.n_text, h0));
      uint32_t ie = h0;
      while (ie < he && fxs_byte(src.text, ie) != ' ') ie++;
      uint32_t is = h0;
      while (is < ie && (fxs_byte(src.text, is) == '>' || fxs_byte(src.text, is) == '@')) is++;
      R.id_off = is; R.id_len = ie - is; R.q_off = 0; R.q_len = 0;
      if (src.fastq) {
        const uint32_t s0 = (uint32_t)src.soff[i];
        const uint32_t plus = min(fxs_find_nl(src.text, src.n_text, s0 + R.readlen) + 1u, src.n_text);
        R.q_off = min(fxs_find_nl(src.text, src.n_text, plus) + 1u, src.n_text);
        R.q_len = fxs_rtrim(src.text, R.q_off, fxs_find_nl(src.text, src.n_text, R.q_off)) - R.q_off;
      }
      meta[i] = make_uint4(R.id_off, R.id_len, R.q_off, R.q_len);
      for (uint32_t k = 0; k < na; k++) {
        const AlignRec a = aln[(size_t)i * slots + k];
        if (!rows_mine(a, o)) continue;
        const uint4 st = stat[(size_t)i * slots + k];
        if (o.want_sam) rows_sam(cs, a, st, R, src, ref, cigar, pool_words, false);
        if (o.want_blast) rows_blast(cb, a, st, R, src, ref, o, cigar, pool_words);
      }
    }
  }
  unsigned long long total;
  const unsigned long long is_ = exp_block_scan(cs.n, s_w, total);
  if (i < rd.n) excl_s[i] = is_ - cs.n;
  if (threadIdx.x == 0) { part_s[blockIdx.x] = total; if (blockIdx.x == 0) part_s[gridDim.x] = 0ull; }
  const unsigned long long ib_ = exp_block_scan(cb.n, s_w, total);
  if (i < rd.n) excl_b[i] = ib_ - cb.n;
  if (threadIdx.x == 0) { part_b[blockIdx.x] = total; if (blockIdx.x == 0) part_b[gridDim.x] = 0ull; }
}

// where the rows of read i begin in their stream (i == n: where the stream ends); part: the exclusive sums of the blocks, the total behind them
__device__ __forceinline__ unsigned long long rows_off(const unsigned long long* __restrict__ excl, const unsigned long long* __restrict__ part, uint32_t n, uint32_t np, uint32_t i) {
  return i >= n ? part[np] : part[i / ROWS_BLOCK] + excl[i];
}

// STREAM 0: the SAM rows, 1: the BLAST rows, which stand behind all SAM rows (one instantiation per stream: each carries one row function)
template <uint32_t STREAM>
__global__ void __launch_bounds__(256) k_rows_write(DReads rd, uint32_t slots, const RState* __restrict__ saved, const AlignRec* __restrict__ aln,
                                                    const uint32_t* __restrict__ cigar, unsigned long long pool_words, const uint4* __restrict__ stat,
                                                    RowsSrc src, RowsRef ref, RowsOpts o, const uint4* __restrict__ meta,
                                                    const unsigned long long* __restrict__ excl, const unsigned long long* __restrict__ part,
                                                    unsigned long long sbase, uint8_t* __restrict__ out) {
  __shared__ __align__(16) uint32_t s_win[4][ROWS_WINDOW / 4 + 16];
  const int lane = lane_id();
  const uint32_t n = rd.n, np = (n + ROWS_BLOCK - 1u) / ROWS_BLOCK;
  const uint32_t n_chunks = (n + 63u) >> 6, n_waves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t chunk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); chunk < n_chunks; chunk += n_waves) {
    const uint32_t i = chunk * 64u + (uint32_t)lane;
    const unsigned long long o0 = sbase + rows_off(excl, part, n, np, min(i, n)), o1 = sbase + rows_off(excl, part, n, np, min(i + 1u, n));
    unsigned long long m = __ballot(o1 != o0);
    if (!m) continue;
    const int r_first = __ffsll((long long)m) - 1, r_last = 63 - __clzll((long long)m);
    RowsWave w;
    w.win = s_win[threadIdx.x >> 6]; w.win8 = reinterpret_cast<uint8_t*>(w.win); w.out = out; w.lane = lane;
    w.first = __shfl(o0, r_first);
    const unsigned long long last = __shfl(o1, r_last);
    w.wbase = w.first & ~3ull; w.pos = w.first;
    while (m) {
      const uint32_t ri = chunk * 64u + (uint32_t)(__ffsll((long long)m) - 1);
      m &= m - 1ull;
      const uint32_t na = min(saved[ri].n_align, slots);
      const uint4 mt = meta[ri];
      RowsRead R;
      R.readlen = rd.len[ri]; R.cw = (R.readlen + 15u) >> 4; R.rec = rd.words + rd.rec_off[ri];
      R.id_off = mt.x; R.id_len = mt.y; R.q_off = mt.z; R.q_len = mt.w;
      uint32_t n_rev = 0;
      for (uint32_t k = 0; k < na; k++) {
        const AlignRec a = aln[(size_t)ri * slots + k];
        if (!rows_mine(a, o)) continue;
        if (!a.strand) n_rev++;
        const uint4 st = stat[(size_t)ri * slots + k];
        if (STREAM == 0u) rows_sam(w, a, st, R, src, ref, cigar, pool_words, (n_rev & 1u) != 0u);
        else rows_blast(w, a, st, R, src, ref, o, cigar, pool_words);
      }
    }
    w.flush();
    // what is left in the window: the bytes of the range's last dword, which the next wave's rows may share
    if (lane == 0) for (unsigned long long b = max(w.wbase, w.first); b < last; b++) out[b] = w.win8[b - w.wbase];
    __threadfence_block();
  }
}

// the seam of the number formatter: out[16 i ..] = rows_fmt(num[i], den[i]), NUL padded
__global__ void k_rows_fmt(uint32_t n, const uint32_t* __restrict__ num, const uint32_t* __restrict__ den, uint8_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const RowsStr s = rows_fmt(num[i], den[i]);
  unsigned long long* const o = reinterpret_cast<unsigned long long*>(out + 16ull * i);
  o[0] = s.lo; o[1] = s.hi;
}

}  // namespace smr
