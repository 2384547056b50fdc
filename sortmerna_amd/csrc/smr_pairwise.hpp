// smr_pairwise.hpp -- the BLAST-like pairwise text of `-blast 0` for the stored alignments of one (index, part), written on the device from what
// smr_rows.hpp reads: the kept FASTX text, the packed letters and ambiguity masks, AlignRec and the CIGAR pool, the part's reference letters,
// the names and the e-value / bit-score table.  The definition of every byte is the do_pair branch of add_rows in smr_report.cpp.
//
// A block of text per alignment: two id lines, the score line (both numbers from the table: no float formatting here), then for every 60
// alignment columns three lines -- "Target:" with the reference letters ('-' at an insertion), the marks ('|' equal, '*' unequal, ' ' at a gap),
// "Query:" with the strand-correct read letters ('-' at a deletion) -- each letter line between its first 1-based position (setw 8 / 9) and the
// running 0-based position behind its last column, as the host prints them.  Where the three lines of a chunk lie depends on the digits of
// these four numbers: pair_plan is the one place that says so, for both kernels.
//
//   k_pair_size   a thread per read (as k_rows_size): where its id lies in the text (meta[]), the bytes of its blocks.  The CIGAR is walked by
//                 operation, never by column: inside an operation the walk steps from chunk boundary to chunk boundary arithmetically.
//   k_pair_write  a wave takes 64 consecutive reads, whose blocks are one contiguous byte range, and puts them together in the LDS window of
//                 RowsWave (smr_rows.hpp; stored by exp_flush as whole dwords, the first and last dword of the range as bytes).  Of a chunk the
//                 wave loads 64 operations from the one its first column lies in; three wave_scan_add give every operation its first column,
//                 reference position and read position.  A first pass finds where the chunk ends and so its four numbers; then lanes write the
//                 fixed bytes of the three lines, and lane c owns column c: it finds its operation by a binary search over the lanes' column
//                 sums (__shfl) and writes its three bytes.  A chunk of more than 64 operations (only zero-length operations make one) and a
//                 CIGAR of more than 64 operations stream through in pieces; a block longer than the window streams through it.  No atomics.
// Both kernels run pair_block over a sink: RowsCount adds lengths, RowsWave writes.  The guards are those of k_rows_stat, launched unchanged.
#pragma once

namespace smr {

#define PAIR_CHUNK 60u

// byte j of v printed right-aligned in w characters (w: at least its digits)
__device__ __forceinline__ uint8_t pair_field(uint32_t v, uint32_t w, uint32_t j) {
  if (j + rows_digits(v) < w) return (uint8_t)' ';
  for (uint32_t k = w - 1u - j; k; k--) v /= 10u;
  return (uint8_t)('0' + v % 10u);
}

// A chunk of n columns whose first column stands at reference position q0 / read position p0 (0-based) and behind whose last column they are
// qe / pe.  Offsets from the chunk's first byte: the Target line is "Target: " + setw(8) of q0 + 1 [t_num characters] + 4 spaces + the letters
// [at lt] + 4 spaces + qe + '\n'; at tl 20 spaces and the marks [at lm]; at qb "\nQuery: " + setw(9) of p0 + 1 [q_num] + 4 spaces + the
// letters [at lq] + 4 spaces + pe + "\n\n".
struct PairPlan { uint32_t n, q1, qe, p1, pe, t_num, dqe, lt, tl, lm, qb, q_num, dpe, lq, total; };
__device__ __forceinline__ PairPlan pair_plan(uint32_t n, uint32_t q0, uint32_t qe, uint32_t p0, uint32_t pe) {
  PairPlan P;
  P.n = n; P.q1 = q0 + 1u; P.qe = qe; P.p1 = p0 + 1u; P.pe = pe;
  P.t_num = max(8u, rows_digits(P.q1)); P.dqe = rows_digits(qe);
  P.lt = 8u + P.t_num + 4u;
  P.tl = P.lt + n + 4u + P.dqe + 1u;
  P.lm = P.tl + 20u;
  P.qb = P.lm + n;
  P.q_num = max(9u, rows_digits(P.p1)); P.dpe = rows_digits(pe);
  P.lq = P.qb + 8u + P.q_num + 4u;
  P.total = P.lq + n + 4u + P.dpe + 2u;
  return P;
}

// ---- the columns, counted: by operation, from chunk boundary to chunk boundary ---------------------------------------------------------------
__device__ __forceinline__ void pair_cols(RowsCount& s, const AlignRec& a, const RowsRead&, const DIndex&, const uint32_t* __restrict__ cigar, unsigned long long pool_words) {
  uint32_t q = (uint32_t)a.ref_begin1, p = (uint32_t)a.read_begin1, q0 = q, p0 = p, fill = 0;
  for (uint32_t k = 0; k < a.cigar_len; k++) {
    const uint32_t c = exp_cigar_word(cigar, pool_words, (unsigned long long)a.cigar_off + k), op = c & 0xFu;
    for (uint32_t len = c >> 4; len;) {
      const uint32_t take = min(len, PAIR_CHUNK - fill);
      if (op != 1u) q += take;
      if (op == 0u || op == 1u) p += take;
      fill += take; len -= take;
      if (fill == PAIR_CHUNK) { s.n += pair_plan(PAIR_CHUNK, q0, q, p0, p).total; q0 = q; p0 = p; fill = 0; }
    }
  }
  if (fill) s.n += pair_plan(fill, q0, q, p0, p).total;
}

// ---- the columns, written ------------------------------------------------------------------------------------------------------------------------
// 64 operations from operation `first` on, one per lane (lane 0: without the `used` columns a previous chunk took of it): len columns of kind
// op, in front of them cs columns, qs reference letters and ps read letters of this piece
struct PairPiece { uint32_t len, op, cs, qs, ps, tot, qtot, ptot; };
__device__ __forceinline__ PairPiece pair_piece(const uint32_t* __restrict__ cigar, unsigned long long pool_words, const AlignRec& a, uint32_t first, uint32_t used, uint32_t lane) {
  PairPiece P;
  const uint32_t k = first + lane;
  const uint32_t c = k < a.cigar_len ? exp_cigar_word(cigar, pool_words, (unsigned long long)a.cigar_off + k) : 0u;
  P.op = c & 0xFu; P.len = (c >> 4) - (lane == 0u ? min(used, c >> 4) : 0u);
  const uint32_t ql = P.op != 1u ? P.len : 0u, pl = (P.op == 0u || P.op == 1u) ? P.len : 0u;
  const uint32_t ce = wave_scan_add(P.len), qe = wave_scan_add(ql), pe = wave_scan_add(pl);
  P.cs = ce - P.len; P.qs = qe - ql; P.ps = pe - pl;
  P.tot = uni((uint32_t)__shfl((int)ce, 63, 64)); P.qtot = uni((uint32_t)__shfl((int)qe, 63, 64)); P.ptot = uni((uint32_t)__shfl((int)pe, 63, 64));
  return P;
}

__device__ __forceinline__ void pair_cols(RowsWave& w, const AlignRec& a, const RowsRead& R, const DIndex& ix, const uint32_t* __restrict__ cigar, unsigned long long pool_words) {
  const uint32_t lane = (uint32_t)w.lane, cnt = a.cigar_len;
  const uint8_t* __restrict__ const refseq = ix.ref_seq + ix.ref_off[a.ref_num];
  uint32_t oi = 0, used = 0, q0 = (uint32_t)a.ref_begin1, p0 = (uint32_t)a.read_begin1;      // the chunk begins in operation oi, `used` columns into it
  while (oi < cnt) {
    const PairPiece first = pair_piece(cigar, pool_words, a, oi, used, lane);
    // where the chunk ends: n columns, dq reference letters, dp read letters; the next one begins in operation noi, nused columns into it
    uint32_t n = 0, dq = 0, dp = 0, noi = cnt, nused = 0;
    {
      PairPiece P = first;
      for (uint32_t o = oi;;) {
        const uint32_t rem = PAIR_CHUNK - n;
        if (P.tot >= rem) {
          const int e = __ffsll((long long)__ballot(P.cs + P.len >= rem)) - 1;
          const uint32_t t = rem - uni((uint32_t)__shfl((int)P.cs, e, 64)), eop = uni((uint32_t)__shfl((int)P.op, e, 64));      // t columns of operation o + e
          dq += uni((uint32_t)__shfl((int)P.qs, e, 64)) + (eop != 1u ? t : 0u);
          dp += uni((uint32_t)__shfl((int)P.ps, e, 64)) + ((eop == 0u || eop == 1u) ? t : 0u);
          noi = o + (uint32_t)e; nused = ((e == 0 && o == oi) ? used : 0u) + t;
          n = PAIR_CHUNK;
          break;
        }
        n += P.tot; dq += P.qtot; dp += P.ptot; o += 64u;
        if (o >= cnt) break;
        P = pair_piece(cigar, pool_words, a, o, 0u, lane);
      }
    }
    if (n == 0u) break;                               // (nothing but operations without columns was left)
    const PairPlan L = pair_plan(n, q0, q0 + dq, p0, p0 + dp);
    w.room(L.total);                                  // (a chunk takes 273 bytes at the most)
    uint8_t* const at = w.win8 + (uint32_t)(w.pos - w.wbase);
    // the fixed bytes of the Target line: up to 22 in front of the letters, up to 15 behind them
    {
      const uint32_t j = lane;
      if (j < 8u) at[j] = (uint8_t)(rows_pack("Target: ") >> (8u * j));
      else if (j < 8u + L.t_num) at[j] = pair_field(L.q1, L.t_num, j - 8u);
      else if (j < L.lt) at[j] = (uint8_t)' ';
      else if (j < L.lt + 4u + L.dqe + 1u) {
        const uint32_t k = j - L.lt;
        at[L.lt + n + k] = k < 4u ? (uint8_t)' ' : (k < 4u + L.dqe ? pair_field(L.qe, L.dqe, k - 4u) : (uint8_t)'\n');
      }
    }
    // the 20 spaces of the marks line; the fixed bytes of the Query line: up to 22 in front of the letters, up to 16 behind them
    {
      const uint32_t j = lane, qf = 8u + L.q_num + 4u;
      if (j < 20u) at[L.tl + j] = (uint8_t)' ';
      else if (j < 28u) at[L.qb + j - 20u] = (uint8_t)(rows_pack("\nQuery: ") >> (8u * (j - 20u)));
      else if (j < 28u + L.q_num) at[L.qb + j - 20u] = pair_field(L.p1, L.q_num, j - 28u);
      else if (j < 20u + qf) at[L.qb + j - 20u] = (uint8_t)' ';
      else if (j < 20u + qf + 4u + L.dpe + 2u) {
        const uint32_t k = j - 20u - qf;
        at[L.lq + n + k] = k < 4u ? (uint8_t)' ' : (k < 4u + L.dpe ? pair_field(L.pe, L.dpe, k - 4u) : (uint8_t)'\n');
      }
    }
    // the columns: lane c has column c of the chunk
    {
      PairPiece P = first;
      uint32_t before = 0, qb = 0, pb = 0;            // columns, reference letters and read letters of the chunk in front of this piece
      for (uint32_t o = oi;;) {
        const uint32_t cl = lane - before;
        const bool mine = lane < n && lane >= before && cl < P.tot;
        const uint32_t x = mine ? cl : 0u, ce = P.cs + P.len;
        uint32_t e = 0;                               // the first operation of the piece that ends behind column x
        for (uint32_t step = 32u; step; step >>= 1) if ((uint32_t)__shfl((int)ce, (int)(e + step - 1u), 64) <= x) e += step;
        e = min(e, 63u);
        const uint32_t ecs = (uint32_t)__shfl((int)P.cs, (int)e, 64), eqs = (uint32_t)__shfl((int)P.qs, (int)e, 64), eps = (uint32_t)__shfl((int)P.ps, (int)e, 64),
                       eop = (uint32_t)__shfl((int)P.op, (int)e, 64);
        if (mine) {
          const uint32_t t = x - ecs;
          uint32_t rc = '-', qc = '-';
          if (eop != 1u) rc = (uint32_t)(0x4E54474341ull >> (8u * min((uint32_t)refseq[q0 + qb + eqs + t], 4u))) & 0xFFu;                          // "ACGTN"
          if (eop == 0u || eop == 1u) qc = (uint32_t)(0x4E54474341ull >> (8u * rows_letter(R.rec, R.cw, R.readlen, a.strand, p0 + pb + eps + t))) & 0xFFu;
          at[L.lt + lane] = (uint8_t)rc;
          at[L.lm + lane] = (uint8_t)(eop != 0u ? ' ' : (rc == qc ? '|' : '*'));
          at[L.lq + lane] = (uint8_t)qc;
        }
        before += P.tot; qb += P.qtot; pb += P.ptot; o += 64u;
        if (before >= n || o >= cnt) break;
        P = pair_piece(cigar, pool_words, a, o, 0u, lane);
      }
    }
    w.pos += L.total;
    q0 += dq; p0 += dp; oi = noi; used = nused;
  }
}

// ---- a block, for either sink --------------------------------------------------------------------------------------------------------------------
template <class S> __device__ __forceinline__ void pair_block(S& s, const AlignRec& a, const RowsRead& R, const RowsSrc& src, const RowsRef& ref, const DIndex& ix,
                                                              const uint32_t* __restrict__ cigar, unsigned long long pool_words) {
  uint32_t no, nl;
  rows_ref_name(ref, a.ref_num, no, nl);
  const uint32_t te = (uint32_t)a.score1 * ROWS_TAB_ENTRY;
  ROWS_LIT(s, "Sequence"); ROWS_LIT(s, " ID: ");
  s.text(ref.names, no, nl, false);
  ROWS_LIT(s, "\nQuery I"); ROWS_LIT(s, "D: ");
  s.text(src.text, R.id_off, R.id_len, false);
  ROWS_LIT(s, "\nScore: ");
  s.str(rows_num((long long)a.score1));
  ROWS_LIT(s, " bits (");
  s.text(ref.tab, te + 16u, fxs_byte(ref.tab, te + 1u), false);
  ROWS_LIT(s, ")\tExpect"); ROWS_LIT(s, ": ");
  s.text(ref.tab, te + 2u, fxs_byte(ref.tab, te), false);
  ROWS_LIT(s, "\tstrand:");
  if (a.strand) ROWS_LIT(s, " +\n\n"); else ROWS_LIT(s, " -\n\n");
  pair_cols(s, a, R, ix, cigar, pool_words);
}

// ---- kernels -------------------------------------------------------------------------------------------------------------------------------------
// excl[i]: the bytes of the blocks of the block's reads in front of read i; part[b]: block b's bytes (entry np: 0, for the scan to leave the
// total there); meta[i] = {offset and length of the id in the text, 0, 0}
__global__ void __launch_bounds__(ROWS_BLOCK) k_pair_size(DReads rd, DIndex ix, uint32_t slots, const RState* __restrict__ saved, const AlignRec* __restrict__ aln,
                                                          const uint32_t* __restrict__ cigar, unsigned long long pool_words, RowsSrc src, RowsRef ref, RowsOpts o,
                                                          uint4* __restrict__ meta, unsigned long long* __restrict__ excl, unsigned long long* __restrict__ part) {
  __shared__ unsigned long long s_w[16];
  const uint32_t i = blockIdx.x * ROWS_BLOCK + threadIdx.x;
  RowsCount cb; cb.n = 0;
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
      meta[i] = make_uint4(R.id_off, R.id_len, 0u, 0u);
      for (uint32_t k = 0; k < na; k++) {
        const AlignRec a = aln[(size_t)i * slots + k];
        if (rows_mine(a, o)) pair_block(cb, a, R, src, ref, ix, cigar, pool_words);
      }
    }
  }
  unsigned long long total;
  const unsigned long long incl = exp_block_scan(cb.n, s_w, total);
  if (i < rd.n) excl[i] = incl - cb.n;
  if (threadIdx.x == 0) { part[blockIdx.x] = total; if (blockIdx.x == 0) part[gridDim.x] = 0ull; }
}

__global__ void __launch_bounds__(256) k_pair_write(DReads rd, DIndex ix, uint32_t slots, const RState* __restrict__ saved, const AlignRec* __restrict__ aln,
                                                    const uint32_t* __restrict__ cigar, unsigned long long pool_words, RowsSrc src, RowsRef ref, RowsOpts o,
                                                    const uint4* __restrict__ meta, const unsigned long long* __restrict__ excl, const unsigned long long* __restrict__ part,
                                                    uint8_t* __restrict__ out) {
  __shared__ __align__(16) uint32_t s_win[4][ROWS_WINDOW / 4 + 16];
  const int lane = lane_id();
  const uint32_t n = rd.n, np = (n + ROWS_BLOCK - 1u) / ROWS_BLOCK;
  const uint32_t n_chunks = (n + 63u) >> 6, n_waves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t chunk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); chunk < n_chunks; chunk += n_waves) {
    const uint32_t i = chunk * 64u + (uint32_t)lane;
    const unsigned long long o0 = rows_off(excl, part, n, np, min(i, n)), o1 = rows_off(excl, part, n, np, min(i + 1u, n));
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
      R.id_off = mt.x; R.id_len = mt.y; R.q_off = 0; R.q_len = 0;
      for (uint32_t k = 0; k < na; k++) {
        const AlignRec a = aln[(size_t)ri * slots + k];
        if (rows_mine(a, o)) pair_block(w, a, R, src, ref, ix, cigar, pool_words);
      }
    }
    w.flush();
    // what is left in the window: the bytes of the range's last dword, which the next wave's blocks may share
    if (lane == 0) for (unsigned long long b = max(w.wbase, w.first); b < last; b++) out[b] = w.win8[b - w.wbase];
    __threadfence_block();
  }
}

}  // namespace smr
