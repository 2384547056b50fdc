// smr_otu_mates.hpp -- the members of otu_map.txt for mates that were read from two files: read i of the selected batch (A) is mate 1 of pair
// i, read i of the mates' batch (B) its mate 2 (smr_otu_part_mates; host side in smr_engine_otu.hpp).  k_otu_classify and k_otu_size of
// smr_otu.hpp run over either batch unchanged; the sort, k_otu_wsize, k_otu_groups and k_otu_gcount see keys and lengths only and run over the
// merged members unchanged.  What is new:
//
//   k_otu_mates_pairs  k_otu_pairs over both batches (blockIdx.y: the batch), a thread per read.  With a[i] / b[i] the passing slots in front of
//                      read i in A / B (otu_off of the two size outputs), the members of A's read i go to a[i] + b[i], those of B's read i to
//                      a[i + 1] + b[i]: pair order, mate 1 before mate 2, then slot order -- the order in which smr_report_add_pair calls add_otu.
//                      No atomics.  A member of B carries OTU_MATE_BIT in its read number.
//   k_otu_mates_write  k_otu_write with two texts: the id of a member with OTU_MATE_BIT is read from B's text, through the same RowsWave window.
//                      A sibling and not an instantiation of one body: k_otu_write's registers are pinned, and the shared body moved them.
#pragma once

namespace smr {

#define OTU_MATE_BIT 0x80000000u          // in uint4::y (the read number) of a member: its id lies in the text of the mates' batch

// what k_otu_mates_pairs reads of one batch: its stored alignments, the pass bits, and the output of k_otu_size
struct OtuSide {
  uint32_t slots;
  const RState* saved; const AlignRec* aln; const uint8_t* pass;
  const uint2* meta; const unsigned long long* excl; const unsigned long long* parts;
};

__global__ void __launch_bounds__(OTU_BLOCK) k_otu_mates_pairs(uint32_t n, OtuSide A, OtuSide B, uint32_t index_num, uint32_t part, uint32_t* __restrict__ keys,
                                                               uint4* __restrict__ pairs) {
  const uint32_t i = blockIdx.x * OTU_BLOCK + threadIdx.x, np = (n + OTU_BLOCK - 1u) / OTU_BLOCK;
  if (i >= n) return;
  const bool mate = blockIdx.y != 0u;
  const unsigned long long a0 = otu_off(A.excl, A.parts, n, np, i), a1 = otu_off(A.excl, A.parts, n, np, i + 1u);
  const unsigned long long b0 = otu_off(B.excl, B.parts, n, np, i), b1 = otu_off(B.excl, B.parts, n, np, i + 1u);
  if ((mate ? b1 - b0 : a1 - a0) == 0ull) return;      // (also: a read whose c_yid_ycov is 0, a batch on which the pass never ran)
  unsigned long long at = (mate ? a1 : a0) + b0;
  const OtuSide& S = mate ? B : A;
  const uint2 mt = S.meta[i];
  const uint32_t na = min(S.saved[i].n_align, S.slots), tag = mate ? i | OTU_MATE_BIT : i;
  for (uint32_t k = 0; k < na; k++) {
    const AlignRec& a = S.aln[(size_t)i * S.slots + k];
    if (a.index_num == index_num && a.part == part && S.pass[(size_t)i * S.slots + k]) { keys[at] = a.ref_num; pairs[at] = make_uint4(a.ref_num, tag, mt.x, mt.y); at++; }
  }
}

__global__ void __launch_bounds__(256) k_otu_mates_write(uint32_t m, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ perm, const uint4* __restrict__ pairs,
                                                         const uint8_t* __restrict__ text, const uint8_t* __restrict__ text_m,
                                                         const unsigned long long* __restrict__ wexcl, const unsigned long long* __restrict__ wparts,
                                                         uint8_t* __restrict__ out) {
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
      w.text((p.y & OTU_MATE_BIT) ? text_m : text, p.z, p.w, false);      // (kk, and with it the text, is the wave's)
      if (kk + 1u < m && keys[kk + 1u] == keys[kk]) ROWS_LIT(w, "\t");
    }
    w.flush();
    // what is left in the window: the bytes of the range's last dword, which the next wave's ids may share
    if (lane == 0) for (unsigned long long b = max(w.wbase, w.first); b < last; b++) out[b] = w.win8[b - w.wbase];
    __threadfence_block();
  }
}

}  // namespace smr
