// smr_nbmap.hpp -- which half-seed searches of k_seed_pg can accept anything at all: one bit per (mini-trie, pattern), built once per index part.
//
// Whether a search finds a string depends on the index part, the key, the direction and the pw pattern chars only -- not on the batch --, and
// on the bench workload 92 % of the searches find none.  Bit [2 * key + DIR][proj(P)] is set iff some string T of the mini-trie has
// lev1_entry(P', T, pw) & 1 for some P' with proj(P') == proj(P); proj keeps the first pw - drop chars of the pattern (drop = 0: the exact
// set).  A set bit says "search", so a false positive costs time and nothing else; a clear bit must never hide a hit.  The patterns a string T
// (pw + 1 chars) accepts are, from the three clauses of lev1_entry with a = the common prefix:
//   T[0..pw-1] with at most one char substituted                      (nothing differs behind char a)            1 + 3 pw
//   T with one of its pw + 1 chars removed                            (P[i] == T[i+1] from char a on)            pw + 1
//   T[0..pw-2] with one free char put in at position 0 .. pw-1        (P[i+1] == T[i] from char a on)            4 pw
// -- 8 pw + 2 candidates per string, some of them equal.  The builder does not trust the list: every candidate goes through lev1_entry itself
// before its bit is set (tests/test_nbmap_enumeration.py: the list is complete, for every (P, T) of pw = 4, 5 and sampled for pw = 9, 10).
#pragma once

namespace smr {

#define NB_MIN_CHARS 4u                                   // fewer pattern chars than this decide nothing: no bitmap
#define NB_MAX_CHARS 9u                                   // a slab of 4^9 bits is the 32 KB of LDS a builder block keeps

__host__ __device__ inline uint32_t nb_cands(uint32_t pw) { return 8u * pw + 2u; }
// candidate c < nb_cands(pw) of string T (2 bits per char, char i at bits 2i)
__host__ __device__ inline uint32_t nb_candidate(uint32_t T, uint32_t pw, uint32_t c) {
  const uint32_t m = (1u << (2 * pw)) - 1u;
  if (c == 0) return T & m;
  c -= 1;
  if (c < 3 * pw) return (T & m) ^ ((c % 3u + 1u) << (2 * (c / 3u)));
  c -= 3 * pw;
  if (c < pw + 1) { const uint32_t lo = (1u << (2 * c)) - 1u; return ((T & lo) | ((T >> 2) & ~lo)) & m; }
  c -= pw + 1;
  const uint32_t j = c >> 2, lo = (1u << (2 * j)) - 1u;
  return ((T & lo) | ((c & 3u) << (2 * j)) | ((T & ~lo) << 2)) & m;
}
__host__ __device__ inline uint64_t nb_slab_words(uint32_t pw, uint32_t drop) { return (uint64_t)1 << (2 * (pw - drop) - 5); }

// present mini-tries and their strings: what the auto policy takes the part's density from
__global__ void __launch_bounds__(256) k_nbmap_census(const uint32_t* __restrict__ root3, uint32_t nb, unsigned long long* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool have = i < nb && root3[2 * i] != NONE;
  const unsigned long long n = have ? root3[2 * i + 1] & 0xFFFFFFu : 0u;
  const unsigned long long present = __popcll(__ballot(have));
  unsigned long long sum = n;
  for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (lane_id() == 0 && present) { atomicAdd(&out[0], present); atomicAdd(&out[1], sum); }
}

// One block per (key, DIR) = block table entry i: the slab in LDS, the strings of the block's TA copy (a block without directories has one copy),
// every candidate of every string verified and its projected bit set; then the slab is copied out.  A key without a mini-trie keeps a zero slab.
__global__ void __launch_bounds__(256) k_nbmap_build(const uint32_t* __restrict__ root3, const uint32_t* __restrict__ pg, uint32_t pw, uint32_t drop,
                                                    uint32_t* __restrict__ nbmap) {
  SMR_DYN_LDS(uint32_t, slab);
  const uint32_t i = blockIdx.x, words = (uint32_t)nb_slab_words(pw, drop), pm = (1u << (2 * (pw - drop))) - 1u;
  uint32_t* out = nbmap + (size_t)i * words;
  const uint32_t rx = root3[2 * i], ry = root3[2 * i + 1];
  if (rx == NONE) {
    for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) out[w] = 0;
    return;
  }
  for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) slab[w] = 0;
  __syncthreads();
  const uint32_t n = ry & 0xFFFFFFu, nc = nb_cands(pw);
  const uint32_t* tt = pg_strings_at(pg, rx, ry);
  for (unsigned long long q = threadIdx.x; q < (unsigned long long)n * nc; q += blockDim.x) {
    const uint32_t t = (uint32_t)(q / nc), c = (uint32_t)(q - (unsigned long long)t * nc);
    const uint32_t T = tt[t], P = nb_candidate(T, pw, c);
    if (lev1_entry(P, T, pw) & 1u) { const uint32_t b = P & pm; atomicOr(&slab[b >> 5], 1u << (b & 31u)); }
  }
  __syncthreads();
  for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) out[w] = slab[w];
}

}  // namespace smr
