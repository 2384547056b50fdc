// smr_idcov.hpp -- part of the HIP kernels of libsmr_hip (included by smr_engine.hip): the %id / %coverage pass over the stored alignments
// of one (index, part) -- what the reference does on the CPU in denovo_stats_run (processor.cpp:287-366) with Read::calc_miss_gap_match
// (read.cpp:547-589) per alignment -- next to the reads, reference letters and CIGARs that are in HBM after smr_traceback.
//
//   k_idcov_collect : the alignments of (index_num, part) that have a CIGAR and are not counted yet -> two work lists by CIGAR length
//                     (ballot compaction, one returning atomic per block and list)
//   k_idcov_few     : few long M runs (Illumina: 1 - 3 operations over 150 letters): 16 lanes per alignment, four alignments per wave, the
//                     lanes of a group stride over the letters of each run, 16 letters per lane and step
//   k_idcov_many    : many short runs (5 kb reads: hundreds of operations of a few letters): one alignment per wave, 64 operations at a time,
//                     an inclusive scan of the operation lengths (wave_scan_add) gives every operation its read / reference start
//
// Letters are compared 16 at a time as words: 32 bits of 2-bit read codes + 16 bits of the ambiguity mask (DReads) against 16 reference
// bytes (DIndex.ref_seq) fetched as aligned dwords; a read's ambiguous letter is 4 (the reference calls flip34 first, processor.cpp:330), so it
// equals a reference N and nothing else.  No LDS; per alignment one atomic on the read's counter, per wave (over its whole list) at most four on the batch's.
//
// A QUIRK THAT IS REPRODUCED, NOT FIXED: denovo_stats_run (processor.cpp:329-333) and fill_otu_map2 (otumap.cpp:131-198) never call
// Read::revIntStr() -- only the BLAST / SAM writers do (report_blast.cpp:132, report_sam.cpp:118).  For an alignment on the reverse strand the
// reference therefore compares the reference window with the letters of the FORWARD read at read_begin1 ...; such alignments practically
// never reach a useful %id, and every read of the reference's otu_map.txt is a '+' read.  The kernels read the forward letters whatever
// AlignRec.strand says.
#pragma once
#include <math.h>

namespace smr {

#define IDCOV_DONE 0x10u         // AlignRec.has_cigar: the alignment has been counted (bit 0: it has a CIGAR; 2 / 3 are k_chain's pending marks)
#define IDCOV_FEW_OPS 8u         // CIGARs of up to this many operations go to k_idcov_few

// the decision of denovo_stats_run (processor.cpp:334-355): 0 = id and coverage, 1 = id only, 2 = coverage only, 3 = neither.
// The reference's host compiler evaluates x * 1000.0 + 0.5 as a product and a sum; hipcc would contract them into one fused operation, which
// rounds once instead of twice -- contraction is switched off for this function so that the answer never depends on it.
__device__ __forceinline__ uint32_t idcov_class(uint32_t n_miss, uint32_t n_gap, uint32_t n_match, int32_t read_begin1, int32_t read_end1, uint32_t readlen,
                                                double min_id, double min_cov) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const uint32_t n_tot = n_miss + n_gap + n_match;
  const int32_t span = read_end1 - read_begin1 + 1;
  const double id = (double)n_match / (double)n_tot;
  const double cov = (double)(span < 0 ? -span : span) / (double)readlen;
  const double id1000 = id * 1000.0, cov1000 = cov * 1000.0;
  const double idr = floor(id1000 + 0.5) / 1000.0;
  const double covr = floor(cov1000 + 0.5) / 1000.0;
  const bool is_id = idr >= min_id, is_cov = covr >= min_cov;
  return is_id ? (is_cov ? 0u : 1u) : (is_cov ? 2u : 3u);
}

// equal letters among cnt (1..16) aligned columns: read letters pb .. of record rec (cw code words, then the mask words), reference letters
// ref_seq[qb ..].  The words one past a record / the reference array are allocated (slack of the uploads); what they hold is masked out.
__device__ __forceinline__ uint32_t idcov_chunk(const uint32_t* __restrict__ rec, uint32_t cw, const uint8_t* __restrict__ ref_seq, uint64_t qb, uint32_t pb, uint32_t cnt) {
  const uint32_t w = pb >> 4, s = (pb & 15u) * 2u;
  const uint32_t codes = (uint32_t)((((unsigned long long)rec[w + 1] << 32) | rec[w]) >> s);
  const uint32_t mi = cw + (pb >> 5), ms = pb & 31u;
  const uint32_t amb = (uint32_t)((((unsigned long long)rec[mi + 1] << 32) | rec[mi]) >> ms);
  const uint32_t* rw = reinterpret_cast<const uint32_t*>(ref_seq + (qb & ~3ull));
  const uint32_t sh = (uint32_t)(qb & 3ull) * 8u, need = ((uint32_t)(qb & 3ull) + cnt + 3u) >> 2;
  uint32_t d[5];
#pragma unroll
  for (uint32_t k = 0; k < 5; k++) d[k] = k < need ? rw[k] : 0u;
  uint32_t n_ne = 0;
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t r4 = (uint32_t)((((unsigned long long)d[k + 1] << 32) | d[k]) >> sh);          // four reference letters
    uint32_t x = (codes >> (8u * k)) & 0xFFu;                                                    // four 2-bit codes -> one per byte
    x = (x | (x << 12)) & 0x000F000Fu; x = (x | (x << 6)) & 0x03030303u;
    uint32_t y = (amb >> (4u * k)) & 0xFu;                                                       // four mask bits -> bit 0 of each byte
    y = (y | (y << 14)) & 0x00030003u; y = (y | (y << 7)) & 0x01010101u;
    const uint32_t l4 = (x & ~(y * 3u)) | (y << 2);                                              // ambiguous: 4
    const uint32_t df = l4 ^ r4;                                                                 // letters are 0..4: a difference is below 8
    const uint32_t ne = (df | (df >> 1) | (df >> 2)) & 0x01010101u;
    const uint32_t v = cnt > 4u * k ? min(cnt - 4u * k, 4u) : 0u;                                 // columns of this dword that count
    const uint32_t vm = v >= 4u ? 0x01010101u : (0x01010101u & ((1u << (8u * v)) - 1u));
    n_ne += (uint32_t)__popc(ne & vm);
  }
  return cnt - n_ne;
}

// one M run of len columns by the lanes l0, l0 + ls, ...: 16 columns per lane and step.  Columns beyond the read or beyond the reference
// sequence (no CIGAR of smr_traceback has any) are not fetched and count as mismatches.
__device__ __forceinline__ void idcov_run(const uint32_t* __restrict__ rec, uint32_t cw, uint32_t readlen, const uint8_t* __restrict__ ref_seq, uint64_t ref_end,
                                          uint32_t pb, uint64_t qb, uint32_t len, uint32_t l0, uint32_t ls, uint32_t& n_match, uint32_t& n_miss) {
  uint32_t ok = len;
  ok = pb < readlen ? min(ok, readlen - pb) : 0u;
  ok = qb < ref_end ? (uint32_t)min((unsigned long long)ok, (unsigned long long)(ref_end - qb)) : 0u;
  for (uint32_t off = l0 * 16u; off < ok; off += ls * 16u) {
    const uint32_t cnt = min(16u, ok - off);
    const uint32_t m = idcov_chunk(rec, cw, ref_seq, qb + off, pb + off, cnt);
    n_match += m; n_miss += cnt - m;
  }
  if (l0 == 0) n_miss += len - ok;
}

// where the result of one alignment goes: its class on the read's counter and (by the caller) the batch's, the alignment marked; or, at the
// seam smr_idcov_batch, the four numbers of triple i
__device__ __forceinline__ void idcov_put(uint32_t i, uint32_t slots, AlignRec* __restrict__ aln, uint32_t* __restrict__ per_read, uint32_t* __restrict__ out,
                                          uint32_t n_miss, uint32_t n_gap, uint32_t n_match, uint32_t cls) {
  if (out) { out[4 * (size_t)i] = n_miss; out[4 * (size_t)i + 1] = n_gap; out[4 * (size_t)i + 2] = n_match; out[4 * (size_t)i + 3] = cls; }
  if (per_read) atomicAdd(&per_read[4 * (size_t)(i / slots) + cls], 1u);
  aln[i].has_cigar = (uint8_t)(aln[i].has_cigar | IDCOV_DONE);
}

// the class counts a wave has gathered over its whole list (n4[k] per lane) onto the batch's counter block: at most four atomics per WAVE.
// (One per alignment was the first version: 800 000 atomics on one 128-byte line, 83 per microsecond whatever the CUs do -- the kernel took
// longer than the traceback of the same batch.)
__device__ __forceinline__ void idcov_totals(const uint32_t n4[4], unsigned long long* __restrict__ ctr, int c_first) {
#pragma unroll
  for (uint32_t k = 0; k < 4; k++) {
    const uint32_t t = wave_sum_u32(n4[k]);
    if (lane_id() == 0 && t) atomicAdd(&ctr[c_first + (int)k], (unsigned long long)t);
  }
}

__global__ void k_idcov_collect(uint32_t n, uint32_t slots, const RState* __restrict__ saved, const AlignRec* __restrict__ aln, uint32_t index_num, uint32_t part,
                                uint32_t* __restrict__ few, uint32_t* __restrict__ many, unsigned long long* __restrict__ ctr, int c_n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool mine = false, cig = false, is_few = false;
  if (i < n * slots) {
    const uint32_t r = i / slots, k = i % slots;
    if (k < saved[r].n_align) {
      const AlignRec& a = aln[i];
      mine = a.index_num == index_num && a.part == part && !(a.has_cigar & IDCOV_DONE);
      cig = (a.has_cigar & 1u) != 0 && a.cigar_len != 0;
      is_few = a.cigar_len <= IDCOV_FEW_OPS;
    }
  }
  const unsigned long long nc = __ballot(mine && !cig);
  if (lane_id() == 0 && nc) atomicAdd(&ctr[c_n + 2], (unsigned long long)__popcll(nc));
  const uint32_t of = block_append(&ctr[c_n], mine && cig && is_few);
  const uint32_t om = block_append(&ctr[c_n + 1], mine && cig && !is_few);
  if (mine && cig) { if (is_few) few[of] = i; else many[om] = i; }
}

__global__ void __launch_bounds__(64) k_idcov_few(DReads rd, DIndex ix, const uint32_t* __restrict__ tasks, uint32_t n_tasks, AlignRec* __restrict__ aln,
                                                  const uint32_t* __restrict__ cigar, uint32_t slots, double min_id, double min_cov,
                                                  uint32_t* __restrict__ per_read, uint32_t* __restrict__ out, unsigned long long* __restrict__ ctr, int c_first) {
  const uint32_t lane = (uint32_t)lane_id(), g = lane >> 4, gl = lane & 15u;
  uint32_t n4[4] = {0, 0, 0, 0};
  for (uint32_t t0 = blockIdx.x * 4u; t0 < n_tasks; t0 += gridDim.x * 4u) {
    const bool have = t0 + g < n_tasks;
    const uint32_t i = have ? tasks[t0 + g] : 0u;
    AlignRec a; a.cigar_len = 0;
    if (have) a = aln[i];
    const uint32_t* rec = rd.words; uint32_t cw = 0, readlen = 0; uint64_t qb = 0, ref_end = 0; uint32_t pb = 0;
    if (have) {
      const uint32_t r = i / slots;
      rec = rd.words + rd.rec_off[r]; readlen = rd.len[r]; cw = (readlen + 15u) >> 4;
      pb = (uint32_t)a.read_begin1; qb = ix.ref_off[a.ref_num] + (uint64_t)a.ref_begin1; ref_end = ix.ref_off[a.ref_num + 1];
    }
    uint32_t ncig = have ? a.cigar_len : 0u, maxc = ncig;
    for (int d = 32; d >= 16; d >>= 1) maxc = max(maxc, (uint32_t)__shfl_xor(maxc, d, 64));
    uint32_t n_match = 0, n_miss = 0, n_gap = 0;
    for (uint32_t q = 0; q < maxc; q++) {
      if (q < ncig) {
        const uint32_t c = cigar[(size_t)a.cigar_off + q], op = c & 0xFu, len = c >> 4;
        if (op == 0) { idcov_run(rec, cw, readlen, ix.ref_seq, ref_end, pb, qb, len, gl, 16u, n_match, n_miss); pb += len; qb += len; }
        else { if (op == 1) pb += len; else qb += len; if (gl == 0) n_gap += len; }
      }
    }
    for (int d = 8; d > 0; d >>= 1) { n_match += __shfl_xor(n_match, d, 64); n_miss += __shfl_xor(n_miss, d, 64); n_gap += __shfl_xor(n_gap, d, 64); }
    if (have && gl == 0) {
      const uint32_t cls = idcov_class(n_miss, n_gap, n_match, a.read_begin1, a.read_end1, a.readlen, min_id, min_cov);
      idcov_put(i, slots, aln, per_read, out, n_miss, n_gap, n_match, cls);
      n4[0] += cls == 0; n4[1] += cls == 1; n4[2] += cls == 2; n4[3] += cls == 3;
    }
  }
  idcov_totals(n4, ctr, c_first);
}

__global__ void __launch_bounds__(64) k_idcov_many(DReads rd, DIndex ix, const uint32_t* __restrict__ tasks, uint32_t n_tasks, AlignRec* __restrict__ aln,
                                                   const uint32_t* __restrict__ cigar, uint32_t slots, double min_id, double min_cov,
                                                   uint32_t* __restrict__ per_read, uint32_t* __restrict__ out, unsigned long long* __restrict__ ctr, int c_first) {
  const uint32_t lane = (uint32_t)lane_id();
  uint32_t n4[4] = {0, 0, 0, 0};
  for (uint32_t t = blockIdx.x; t < n_tasks; t += gridDim.x) {
    const uint32_t i = tasks[t];
    const AlignRec a = aln[i];
    const uint32_t r = i / slots, readlen = rd.len[r], cw = (readlen + 15u) >> 4;
    const uint32_t* rec = rd.words + rd.rec_off[r];
    const uint64_t ref_end = ix.ref_off[a.ref_num + 1];
    uint32_t pb0 = (uint32_t)a.read_begin1; uint64_t qb0 = ix.ref_off[a.ref_num] + (uint64_t)a.ref_begin1;
    uint32_t n_match = 0, n_miss = 0, n_gap = 0;
    for (uint32_t q0 = 0; q0 < a.cigar_len; q0 += 64u) {
      const uint32_t q = q0 + lane;
      const uint32_t c = q < a.cigar_len ? cigar[(size_t)a.cigar_off + q] : 0u, op = c & 0xFu, len = c >> 4;
      const uint32_t ra = op == 2 ? 0u : len, fa = op == 1 ? 0u : len;         // letters of the read / of the reference the operation consumes
      const uint32_t ri = wave_scan_add(ra), fi = wave_scan_add(fa);
      if (op == 0) idcov_run(rec, cw, readlen, ix.ref_seq, ref_end, pb0 + ri - ra, qb0 + (fi - fa), len, 0u, 1u, n_match, n_miss);
      else n_gap += len;
      pb0 += (uint32_t)__shfl(ri, 63, 64); qb0 += (uint32_t)__shfl(fi, 63, 64);
    }
    n_match = wave_sum_u32(n_match); n_miss = wave_sum_u32(n_miss); n_gap = wave_sum_u32(n_gap);
    if (lane == 0) {
      const uint32_t cls = idcov_class(n_miss, n_gap, n_match, a.read_begin1, a.read_end1, a.readlen, min_id, min_cov);
      idcov_put(i, slots, aln, per_read, out, n_miss, n_gap, n_match, cls);
      n4[0] += cls == 0; n4[1] += cls == 1; n4[2] += cls == 2; n4[3] += cls == 3;
    }
  }
  idcov_totals(n4, ctr, c_first);
}

// the counters of the reads that smr_results_fetch packed (k_results_compact): packed position -> the read's four
__global__ void k_idcov_gather(const uint32_t* __restrict__ idx, const unsigned long long* __restrict__ n_packed, const uint32_t* __restrict__ per_read, uint32_t* __restrict__ out) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if ((unsigned long long)p >= *n_packed) return;
  const uint32_t r = idx[p];
  for (int k = 0; k < 4; k++) out[4 * (size_t)p + k] = per_read[4 * (size_t)r + k];
}

}  // namespace smr
