// smr_import.hpp -- k_import_state: the stored per-read records (Read::toBinString bytes, what smr_result_record hands out) parsed back into
// RState / AlignRec / the CIGAR pool of a batch, next to where they live (Read::load_db, read.cpp:467-539).
//
// A record (little endian, no padding; record_of in smr_engine.hip writes the same bytes):
//    0 lastIndex u32     4 lastPart u32      8 c_yid_ycov, n_yid_ncov, n_nid_ycov, n_denovo 4 x u32
//   24 is_done u8       25 is_hit u8        26 null_align_output u8 (always written 0, not kept)
//   27 max_SW_count u16 29 num_alignments i32  33 hit_seeds u32  37 alignment_size u64 = record length - 45
//   45 min_index u32    49 max_index u32    53 n_align u64
//   61 per alignment: u64 length of what follows (= 39 + 4 cl), u64 cl, cl x u32 CIGAR, ref_num u32, ref_begin1, ref_end1, read_begin1,
//      read_end1 i32, readlen u32, score1, part, index_num u16, strand u8
// The header is 45 bytes and every alignment adds 47 + 4 cl, so neither records nor fields are 4-byte aligned: every field is put together
// from aligned dwords by a byte funnel shift (imp_u32), no byte loads and no misaligned dword loads.
//
// Work split: a wave takes 64 consecutive reads at a time.  First every lane looks at ITS read: a read without a record is cleared (the
// state of a fresh upload), a record has its length chain walked and every field bounds-checked against the record's end before it is
// loaded (n_align <= slots, so the walk is short).  One prefix sum over the lanes and one atomic on C_CIGAR_CURSOR reserve the CIGAR words of all
// 64 records; the order of CIGARs in the pool is free, the alignments carry their offsets.  Then the wave goes through its valid records one
// by one: lane k < n_align writes alignment k, and all lanes copy the CIGAR words.  Whatever is wrong with a record raises a bit of flag[0] and
// nothing of that record is written; the host then puts the batch back into its fresh state, so no partial import survives.
#pragma once

namespace smr {

enum { IMP_ERR_FORMAT = 1u, IMP_ERR_SLOTS = 2u, IMP_ERR_READLEN = 4u, IMP_ERR_IDCOV = 8u, IMP_ERR_NUMALN = 16u, IMP_ERR_POOL = 32u };
#define IMP_HEADER 61u
#define IMP_ALN_FIXED 47u       // bytes of an alignment without its CIGAR words, the two length fields included

// the four bytes at byte offset o of the record buffer; the caller has checked o + 4 <= the buffer's bytes (the buffer ends on a whole word)
__device__ __forceinline__ uint32_t imp_u32(const uint32_t* __restrict__ w, unsigned long long o) {
  const unsigned long long q = o >> 2;
  const uint32_t s = (uint32_t)o & 3u, lo = w[q], hi = s ? w[q + 1] : 0u;
  return (uint32_t)(((((unsigned long long)hi) << 32) | lo) >> (8u * s));
}
__device__ __forceinline__ unsigned long long imp_u64(const uint32_t* __restrict__ w, unsigned long long o) {
  return (unsigned long long)imp_u32(w, o) | ((unsigned long long)imp_u32(w, o + 4) << 32);
}

// bytes: the caller's bytes [o_base, o_base + n_bytes), off: the caller's offsets.  flag[0]: IMP_ERR_* bits; flag[2..3] as one u64: 0, or 2^32 | the num_alignments field the records agree on
__global__ void __launch_bounds__(256) k_import_state(const uint32_t* __restrict__ bytes, unsigned long long o_base, unsigned long long n_bytes, const unsigned long long* __restrict__ off, uint32_t n,
                                                      uint32_t slots, const uint32_t* __restrict__ len, RState* __restrict__ saved, AlignRec* __restrict__ saved_aln,
                                                      uint32_t* __restrict__ cigar, unsigned long long pool_words, unsigned long long* __restrict__ ctr, uint32_t* __restrict__ flag) {
  const int lane = lane_id();
  const uint32_t n_chunks = (n + 63u) >> 6, n_waves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t chunk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); chunk < n_chunks; chunk += n_waves) {
    const uint32_t i = chunk * 64u + (uint32_t)lane;
    unsigned long long o0 = 0, L = 0;
    uint32_t err = 0, na = 0, numaln = 0;
    unsigned long long words = 0;
    bool rec = false;
    if (i < n) {
      const unsigned long long a0 = off[i], a1 = off[i + 1];          // (the buffer holds bytes [o_base, o_base + n_bytes) of the caller's)
      if (a0 < o_base || a0 > a1 || a1 - o_base > n_bytes) err = IMP_ERR_FORMAT;
      else { o0 = a0 - o_base; L = a1 - a0; rec = L != 0; }
      if (!rec) {                                          // no stored record: what an upload leaves
        const RState z = {};
        saved[i] = z;
        const AlignRec za = {};
        for (uint32_t k = 0; k < slots; k++) saved_aln[(size_t)i * slots + k] = za;
      }
    }
    if (rec) {
      // the length chain, every step inside [o0, o0 + L)
      if (L < IMP_HEADER) err = IMP_ERR_FORMAT;
      else {
        const unsigned long long asz = imp_u64(bytes, o0 + 37), nal = imp_u64(bytes, o0 + 53);
        if (asz != L - 45u) err |= IMP_ERR_FORMAT;
        else if (nal > slots) err |= IMP_ERR_SLOTS;
        else {
          if (imp_u32(bytes, o0 + 8) | imp_u32(bytes, o0 + 12) | imp_u32(bytes, o0 + 16) | imp_u32(bytes, o0 + 20)) err |= IMP_ERR_IDCOV;
          numaln = imp_u32(bytes, o0 + 29);
          na = (uint32_t)nal;
          unsigned long long pos = IMP_HEADER;
          for (uint32_t k = 0; k < na; k++) {
            if (pos + 16u > L) { err |= IMP_ERR_FORMAT; break; }
            const unsigned long long rl = imp_u64(bytes, o0 + pos), cl = imp_u64(bytes, o0 + pos + 8);
            if (cl > (L >> 2) || rl != 4u * cl + (IMP_ALN_FIXED - 8u) || pos + 8u + rl > L) { err |= IMP_ERR_FORMAT; break; }
            if (imp_u32(bytes, o0 + pos + 16u + 4u * cl + 20u) != len[i]) err |= IMP_ERR_READLEN;
            words += cl;
            pos += 8u + rl;
          }
          if (!(err & IMP_ERR_FORMAT) && pos != L) err |= IMP_ERR_FORMAT;      // trailing bytes
        }
      }
    }
    const bool ok = rec && err == 0;
    if (!ok) words = 0;
    // the records of one batch carry one num_alignments (Read::init copies the option into every read)
    const unsigned long long m_ok = __ballot(ok);
    if (m_ok) {
      const int first = __ffsll((long long)m_ok) - 1;
      const uint32_t na0 = __shfl(numaln, first);
      if (ok && numaln != na0) err |= IMP_ERR_NUMALN;
      if (lane == first) {
        const unsigned long long v = (1ull << 32) | na0;
        const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(flag + 2), 0ull, v);
        if (old != 0ull && old != v) err |= IMP_ERR_NUMALN;
      }
    }
    // the CIGAR words of the wave's records: one scan, one atomic
    unsigned long long incl = words;                              // (64-bit sums: offsets that overlap can name more words than the buffer has)
    for (int d = 1; d < 64; d <<= 1) { const unsigned long long t = __shfl_up(incl, (unsigned)d); if (lane >= d) incl += t; }
    const unsigned long long total = __shfl(incl, 63);
    unsigned long long base = 0;
    if (total) {
      if (lane == 0) base = atomicAdd(&ctr[C_CIGAR_CURSOR], total);
      base = __shfl(base, 0);
      if (base + total > pool_words) err |= IMP_ERR_POOL;         // (offsets that overlap: the host sized the pool for records that lie side by side)
    }
    if (err) atomicOr(&flag[0], err);
    unsigned long long m = (total && base + total > pool_words) ? 0ull : m_ok;
    const unsigned long long my_base = base + (incl - words);
    while (m) {
      const int r = __ffsll((long long)m) - 1;
      m &= m - 1;
      const unsigned long long ro = __shfl(o0, r);
      const uint32_t rn = __shfl(na, r), ri = chunk * 64u + (uint32_t)r;
      unsigned long long cb = __shfl(my_base, r);
      if (lane == 0) {
        RState s;
        s.lastIndex = imp_u32(bytes, ro); s.lastPart = imp_u32(bytes, ro + 4);
        const uint32_t f = imp_u32(bytes, ro + 24), g = imp_u32(bytes, ro + 27);      // is_done, is_hit, (null_align_output), max_SW_count
        s.is_done = (uint8_t)(f & 0xFFu); s.is_hit = (uint8_t)((f >> 8) & 0xFFu); s.max_SW_count = (uint16_t)(g & 0xFFFFu);
        s.hit_seeds = imp_u32(bytes, ro + 33); s.min_index = imp_u32(bytes, ro + 45); s.max_index = imp_u32(bytes, ro + 49); s.n_align = rn;
        saved[ri] = s;
      }
      // every lane walks the (validated) chain; lane k keeps alignment k, all copy the CIGAR words
      unsigned long long pos = IMP_HEADER;
      for (uint32_t k = 0; k < rn; k++) {
        const uint32_t cl = imp_u32(bytes, ro + pos + 8);
        const unsigned long long cg = ro + pos + 16u, q = cg + 4ull * cl;
        if ((uint32_t)lane == (k & 63u)) {
          AlignRec a;
          a.ref_num = imp_u32(bytes, q); a.ref_begin1 = (int32_t)imp_u32(bytes, q + 4); a.ref_end1 = (int32_t)imp_u32(bytes, q + 8);
          a.read_begin1 = (int32_t)imp_u32(bytes, q + 12); a.read_end1 = (int32_t)imp_u32(bytes, q + 16); a.readlen = imp_u32(bytes, q + 20);
          const uint32_t sp = imp_u32(bytes, q + 24), is = imp_u32(bytes, q + 27);   // score1, part | (part >> 8), index_num, strand
          a.score1 = (uint16_t)(sp & 0xFFFFu); a.part = (uint16_t)(sp >> 16); a.index_num = (uint16_t)((is >> 8) & 0xFFFFu); a.strand = (uint8_t)(is >> 24);
          a.has_cigar = cl ? 1 : 0; a.cigar_off = cl ? (uint32_t)cb : 0u; a.cigar_len = cl;
          saved_aln[(size_t)ri * slots + k] = a;
        }
        for (uint32_t j = (uint32_t)lane; j < cl; j += 64u) cigar[cb + j] = imp_u32(bytes, cg + 4ull * j);
        cb += cl;
        pos += IMP_ALN_FIXED + 4ull * cl;
      }
      // the slots behind the stored alignments: as after an upload
      for (uint32_t k = rn + (uint32_t)lane; k < slots; k += 64u) { const AlignRec za = {}; saved_aln[(size_t)ri * slots + k] = za; }
    }
  }
}

}  // namespace smr
