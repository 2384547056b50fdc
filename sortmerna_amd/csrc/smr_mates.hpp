// smr_mates.hpp -- k_mates_zip: the row streams of two batches whose reads are mates (read i of batch A, read i of batch B) interleaved on the
// device into the order in which the host writer appends them (smr_report_add_pair: mate 1 of pair 0, mate 2 of pair 0, mate 1 of pair 1, ...).
//
// With a[i] / b[i] the exclusive byte offsets of read i in A's / B's stream (a[n], b[n]: the totals)
//   the rows of A's read i go to a[i] + b[i],  the rows of B's read i go to a[i + 1] + b[i],
// so no further scan is needed: the offsets are what k_rows_size / k_pair_size left on the device (excl[i] + part[i / ROWS_BLOCK]).
//
// Logical piece p is the byte range of read p / 2 of A (p even) or of B (p odd); most pieces are empty.  A wave takes a group of MATES_GROUP
// consecutive pairs, whose output range [a[i0] + b[i0], a[i1] + b[i1]) is contiguous, as are its two source ranges.  When no piece of the
// group is longer than MATES_TEAM_BYTES, the wave's four teams of MATES_TEAM lanes take MATES_TEAM consecutive pairs each, else the whole wave
// takes the group; either way a team walks the pieces that are not empty, in order, and keeps the output position and the bytes of the dword
// that is not yet full (FxsOut of smr_fxsplit.hpp, the same in every lane).  A piece goes out as k_fxs_copy puts its pieces out: the bytes
// that fill the open dword, then whole dwords, lane after lane, each put together from two aligned source dwords by a byte funnel
// (v_perm_b32) and stored once, then the piece's last bytes into the open dword -- which the next piece of the team completes.  Only the first
// and the last dword of a TEAM's range can hold bytes of a neighbouring team or wave: of such a dword the team stores its own bytes only, as
// bytes.  No atomics, no LDS, nothing stored at or behind a[n] + b[n]; a source is read up to 7 bytes behind its last byte (its buffer is
// padded by 8).
#pragma once

namespace smr {

#define MATES_GROUP 64u          // pairs per wave and round of the grid-stride loop
#define MATES_TEAM 16u           // lanes of a team, and the consecutive pairs it takes
#define MATES_TEAM_BYTES 1024u   // a piece longer than this is streamed through by the whole wave (and with it its group)

// one row stream as its size kernel left it: piece i is bytes[base + off(i), base + off(i + 1))
struct MatesSrc {
  const uint8_t* bytes; unsigned long long base;
  const unsigned long long* excl; const unsigned long long* part;      // off(i) = part[i / ROWS_BLOCK] + excl[i]; part[np] = the total
};
__device__ __forceinline__ unsigned long long mates_off(const MatesSrc& s, uint32_t n, uint32_t np, uint32_t i) { return rows_off(s.excl, s.part, n, np, i); }

// the four bytes at p, whatever its phase: two aligned dwords and a byte funnel
__device__ __forceinline__ uint32_t mates_load4(const uint8_t* __restrict__ src, unsigned long long p) {
  const uint32_t* const t32 = reinterpret_cast<const uint32_t*>(src) + (p >> 2);
  return perm_b32(t32[1], t32[0], 0x03020100u + 0x01010101u * ((uint32_t)p & 3u));
}
// appends src[s, s + L); lane tl of a team of W (fxs_append with 64-bit source offsets and lengths)
__device__ __forceinline__ void mates_append(FxsOut& w, const uint8_t* __restrict__ src, unsigned long long s, unsigned long long L, uint32_t tl, uint32_t W) {
  if (L == 0ull) return;
  const uint32_t head = (uint32_t)min(L, (unsigned long long)((4u - ((uint32_t)w.pos & 3u)) & 3u));
  if (head) fxs_put(w, mates_load4(src, s), head, tl == 0u);
  const unsigned long long nd = (L - head) >> 2;
  if (nd) {                                                     // (pos is on a dword now and nothing is open)
    uint32_t* const o32 = reinterpret_cast<uint32_t*>(w.out) + (w.pos >> 2);
    for (unsigned long long j = tl; j < nd; j += W) o32[j] = mates_load4(src, s + head + 4ull * j);
    w.pos += 4ull * nd;
  }
  const uint32_t tail = (uint32_t)(L - head - 4ull * nd);
  if (tail) fxs_put(w, mates_load4(src, s + L - tail), tail, tl == 0u);
}

__global__ void __launch_bounds__(256) k_mates_zip(uint32_t n, MatesSrc a, MatesSrc b, unsigned long long obase, uint8_t* __restrict__ out) {
  const uint32_t lane = (uint32_t)lane_id();
  const uint32_t np = (n + ROWS_BLOCK - 1u) / ROWS_BLOCK;
  const uint32_t n_groups = (n + MATES_GROUP - 1u) / MATES_GROUP, n_waves = gridDim.x * (blockDim.x >> 6);
  for (uint32_t g = uni(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); g < n_groups; g += n_waves) {      // (uni: the ends of a group are scalar loads)
    const uint32_t i0 = g * MATES_GROUP, i1 = min(n, i0 + MATES_GROUP);
    // an empty group: its two ends, and on
    if (mates_off(a, n, np, i0) + mates_off(b, n, np, i0) == mates_off(a, n, np, i1) + mates_off(b, n, np, i1)) continue;
    const uint32_t i = min(i0 + lane, n);
    const unsigned long long la = mates_off(a, n, np, min(i + 1u, n)) - mates_off(a, n, np, i), lb = mates_off(b, n, np, min(i + 1u, n)) - mates_off(b, n, np, i);
    const unsigned long long m = __ballot(la != 0ull || lb != 0ull);
    const bool wide = __any(la > MATES_TEAM_BYTES || lb > MATES_TEAM_BYTES);
    const uint32_t W = wide ? 64u : MATES_TEAM, tl = lane & (W - 1u);
    const uint32_t t0 = wide ? i0 : i0 + (lane & ~(MATES_TEAM - 1u));          // the team's first pair
    unsigned long long mk = wide ? m : (m >> (lane & ~(MATES_TEAM - 1u))) & ((1ull << MATES_TEAM) - 1ull);
    if (!mk) continue;
    FxsOut w;
    w.out = out; w.open = 0u;
    {                                                                          // (pairs without bytes in front of the first piece move nothing)
      const uint32_t f = t0 + (uint32_t)(__ffsll((long long)mk) - 1);
      w.first = w.pos = obase + mates_off(a, n, np, f) + mates_off(b, n, np, f);
    }
    while (mk) {
      const uint32_t r = t0 + (uint32_t)(__ffsll((long long)mk) - 1);
      mk &= mk - 1ull;
      const unsigned long long a0 = mates_off(a, n, np, r), a1 = mates_off(a, n, np, r + 1u), b0 = mates_off(b, n, np, r), b1 = mates_off(b, n, np, r + 1u);
      mates_append(w, a.bytes, a.base + a0, a1 - a0, tl, W);
      mates_append(w, b.bytes, b.base + b0, b1 - b0, tl, W);
    }
    // the team's last bytes: the dword they lie in can be the next team's as well
    if (tl == 0u) for (unsigned long long q = max(w.pos & ~3ull, w.first); q < w.pos; q++) out[q] = (uint8_t)(w.open >> (8u * (uint32_t)(q & 3ull)));
  }
}

}  // namespace smr
