// smr_engine_swseam.hpp -- the Smith-Waterman kernels at the ssw.h seam (included by smr_engine.hip): the device self-check of the packed kernels, smr_ssw_batch, smr_sw16_batch, smr_sw_mode,
// smr_walk_rounds.
// (one translation unit: no include guard games -- this file is text of smr_engine.hip, cut out along its stages)

// =================================================================================================
// Device self-check of the packed Smith-Waterman kernel against the 32-bit one (both on the GPU): one wave per case, seeded
// pseudo-random read (1..max_m nt, ~1.5 % N) against either a mutated copy of it with substitutions and indels or a random
// sequence; forward pass and the reverse-direction pass on the prefixes ending in the forward end cell, like k_chain's two calls.
__device__ __forceinline__ uint32_t sc_hash(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA6Bu ^ (c + 0x165667B1u) * 0xC2B2AE35u;
  h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
  return h;
}
__global__ void __launch_bounds__(64) k_sw_selfcheck(uint32_t n_cases, uint32_t seed, uint32_t max_m, uint32_t lds_m, uint32_t lds_n,
                                                     int match, int mismatch, int scoreN, int go, int ge, int mode_b, unsigned long long* out) {
  SMR_DYN_LDS(unsigned char, lds_raw);
  uint8_t* rdq = lds_raw;
  uint8_t* rfq = rdq + lds_m;
  int* bound = (int*)(rfq + lds_n);
  __shared__ int s_n;
  const int lane = smr::lane_id();
  for (uint32_t cs = blockIdx.x; cs < n_cases; cs += gridDim.x) {
    const uint32_t hm = sc_hash(seed, cs, 1);
    const int m = 1 + (int)(hm % max_m);
    for (int q = lane; q < m; q += 64) { const uint32_t h = sc_hash(seed, cs, 100u + (uint32_t)q); rdq[q] = (h & 63u) == 0 ? 4 : (uint8_t)((h >> 8) & 3u); }
    __syncthreads();
    if (lane == 0) {
      int n = 0;
      const bool homolog = (hm >> 20) & 3u;                       // 3 of 4 cases: a mutated copy (with a random flank), else unrelated
      const int flank = (int)((hm >> 24) & 15u);
      for (int q = 0; q < flank; q++) rfq[n++] = (uint8_t)(sc_hash(seed, cs, 5000u + (uint32_t)q) & 3u);
      for (int q = 0; q < m && n + 2 < (int)lds_n; q++) {
        const uint32_t h = sc_hash(seed, cs, 9000u + (uint32_t)q);
        if (!homolog) { rfq[n++] = (uint8_t)(h & 3u); continue; }
        const uint32_t ev = (h >> 4) & 63u;
        if (ev == 0) continue;                                      // deletion in the reference
        if (ev == 1) rfq[n++] = (uint8_t)((h >> 12) & 3u);          // insertion
        if (ev == 2) { rfq[n++] = 4; continue; }                    // N in the reference
        rfq[n++] = ev < 6 ? (uint8_t)((h >> 16) & 3u) : (rdq[q] == 4 ? (uint8_t)0 : rdq[q]);
      }
      for (int q = 0; q < flank && n + 1 < (int)lds_n; q++) rfq[n++] = (uint8_t)(sc_hash(seed, cs, 7000u + (uint32_t)q) & 3u);
      s_n = n;
    }
    __syncthreads();
    const int n = s_n;
    const smr::SwRes a0 = smr::sw_wave(rdq, m, 0, 1, rfq, n, 0, 1, bound, match, mismatch, scoreN, go, ge, 0);
    __syncthreads();
    const smr::SwRes a1 = smr::sw_wave(rdq, m, 0, 1, rfq, n, 0, 1, bound, match, mismatch, scoreN, go, ge, mode_b);
    __syncthreads();
    bool bad = a0.score != a1.score || a0.end_ref != a1.end_ref || a0.end_read != a1.end_read;
    if (a0.score > 0 && a0.end_ref >= 0) {
      const smr::SwRes b0 = smr::sw_wave(rdq, a0.end_read + 1, a0.end_read, -1, rfq, a0.end_ref + 1, a0.end_ref, -1, bound, match, mismatch, scoreN, go, ge, 0);
      __syncthreads();
      const smr::SwRes b1 = smr::sw_wave(rdq, a0.end_read + 1, a0.end_read, -1, rfq, a0.end_ref + 1, a0.end_ref, -1, bound, match, mismatch, scoreN, go, ge, mode_b);
      __syncthreads();
      bad = bad || b0.score != b1.score || b0.end_ref != b1.end_ref || b0.end_read != b1.end_read;
    }
    if (lane == 0) { atomicAdd(&out[0], 1ull); if (bad) atomicAdd(&out[1], 1ull); atomicAdd(&out[2], (unsigned long long)a0.score); }
    __syncthreads();
  }
}

extern "C" int smr_sw_selfcheck(smr_ctx* c, uint32_t n_cases, uint32_t seed, uint32_t max_len, uint64_t* n_bad) {
  if (!c || !n_bad || max_len == 0 || max_len > 4000) return SMR_ERR_ARG;
  (void)hipSetDevice(c->device);
  DevPool pool;
  IB_GET(d, unsigned long long, 3);
  HIPCHK(c, hipMemsetAsync(d, 0, 3 * 8, c->stream));
  const uint32_t lm = (max_len + 15) & ~15u, ln = (max_len + max_len / 16 + 64 + 15) & ~15u;
  const size_t lds = (size_t)lm + ln + (size_t)2 * ln * 4;
  const int sc[2][3] = {{2, -3, -3}, {5, -4, -4}};
  for (int k = 0; k < 2 && n_cases; k++)
    hipLaunchKernelGGL(k_sw_selfcheck, dim3(std::min<uint32_t>(n_cases, (uint32_t)c->n_cu * 8u)), dim3(64), lds, c->stream, n_cases, seed + 7919u * (uint32_t)k, max_len, lm, ln,
                       sc[k][0], sc[k][1], sc[k][2], 5, 2, std::max(c->sw_mode, 1), d);
  unsigned long long h[3] = {0, 0, 0};
  HIPCHK(c, hipMemcpyAsync(h, d, 3 * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (h[0] != 2ull * n_cases) { set_err(c, "SW self-check did not run all cases"); return SMR_ERR_DEVICE; }
  *n_bad = h[1];
  return SMR_OK;
}


// =================================================================================================
// Batched Smith-Waterman at the ssw.h seam (SURVEY.md 8b "existing C ABI"): what k_chain does per candidate -- ssw_align(prof, ref,
// refLen, gapO, gapE, flag = 2, filters, 0, 0) (ssw.c:834-941) without the CIGAR -- for n independent (read, reference window) pairs,
// one wave per pair.  A unit-test surface for the SW kernels against the reference's own ssw.c (tests/golden/ssw_pairs.json).
// =================================================================================================
// A pair without any positive cell: the kernels return {0, -1, m - 1}, a value none of their callers reads (a score of 0 is never accepted); ssw_align
// returns read_end1 = 0 for it (its scan for the end row meets a column of zeros, ssw.c:329-335), and that is what the seam reports.
__device__ __forceinline__ int ssw_end_read(const smr::SwRes& fw) { return fw.score > 0 ? fw.end_read : 0; }
template <bool STRIPED>
__global__ void __launch_bounds__(64) k_ssw_batch(uint32_t n_pairs, const uint8_t* __restrict__ reads, const unsigned long long* __restrict__ read_off,
                                                  const uint8_t* __restrict__ refs, const unsigned long long* __restrict__ ref_off, uint32_t lds_m, uint32_t lds_n,
                                                  int match, int mismatch, int scoreN, int go, int ge, uint32_t filters, int mode, int* __restrict__ out, uint16_t* scr_all, uint32_t scr_stride) {
  SMR_DYN_LDS(unsigned char, lds_raw);
  uint8_t* rdq = lds_raw;
  uint8_t* rfq = rdq + lds_m;
  int* bound = (int*)(rfq + lds_n);
  uint16_t* scr = scr_all ? scr_all + (size_t)blockIdx.x * scr_stride : nullptr;      // (mode < 0: the striped slow path)
  const int lane = smr::lane_id();
  for (uint32_t pi = blockIdx.x; pi < n_pairs; pi += gridDim.x) {
    const int m = (int)(read_off[pi + 1] - read_off[pi]), n = (int)(ref_off[pi + 1] - ref_off[pi]);
    for (int q = lane; q < m; q += 64) rdq[q] = reads[read_off[pi] + q];
    for (int q = lane; q < n; q += 64) rfq[q] = refs[ref_off[pi] + q];
    __syncthreads();
    int res[5] = {0, -1, -1, -1, m - 1};          // score1, ref_begin1, ref_end1, read_begin1, read_end1
    if (m > 0 && n > 0) {
      const smr::SwRes fw = smr::sw_wave_t<STRIPED>(rdq, m, 0, 1, rfq, n, 0, 1, bound, match, mismatch, scoreN, go, ge, mode, 0, 0, scr);
      __syncthreads();
      res[0] = fw.score > 65535 ? 65535 : fw.score; res[2] = fw.end_ref; res[4] = ssw_end_read(fw);
      if ((uint32_t)res[0] >= filters && fw.score > 0) {
        const smr::SwRes bw = smr::sw_wave_t<STRIPED>(rdq, fw.end_read + 1, fw.end_read, -1, rfq, fw.end_ref + 1, fw.end_ref, -1, bound, match, mismatch, scoreN, go, ge, mode, res[0], fw.word, scr);
        __syncthreads();
        res[1] = fw.end_ref - bw.end_ref; res[3] = fw.end_read - bw.end_read;
      }
    }
    if (lane < 5) out[(size_t)pi * 5 + lane] = res[lane];
    __syncthreads();
  }
}

// mode 5: through sw_wave_any_t, the entry k_chain<LONG> and k_begins<LONG> use (spans of more than 512 rows take the strips of sw_wave_long).  A kernel of
// its own with their three waves per SIMD: the strips are noinline functions shared with them, and the compiler gives such a function the loosest
// register budget among its callers (without the bound here k_chain<LONG> went from 168 to 280 registers: tests/test_kernel_resources.py).
__global__ void __launch_bounds__(64, 3) k_ssw_long(uint32_t n_pairs, const uint8_t* __restrict__ reads, const unsigned long long* __restrict__ read_off,
                                                   const uint8_t* __restrict__ refs, const unsigned long long* __restrict__ ref_off, uint32_t lds_m, uint32_t lds_n,
                                                   int match, int mismatch, int scoreN, int go, int ge, uint32_t filters, int* __restrict__ out) {
  SMR_DYN_LDS(unsigned char, lds_raw);
  uint8_t* rdq = lds_raw;
  uint8_t* rfq = rdq + lds_m;
  int* bound = (int*)(rfq + lds_n);
  const int lane = smr::lane_id();
  for (uint32_t pi = blockIdx.x; pi < n_pairs; pi += gridDim.x) {
    const int m = (int)(read_off[pi + 1] - read_off[pi]), n = (int)(ref_off[pi + 1] - ref_off[pi]);
    for (int q = lane; q < m; q += 64) rdq[q] = reads[read_off[pi] + q];
    for (int q = lane; q < n; q += 64) rfq[q] = refs[ref_off[pi] + q];
    __syncthreads();
    int res[5] = {0, -1, -1, -1, m - 1};
    if (m > 0 && n > 0) {
      const smr::SwRes fw = smr::sw_wave_any_t<false>(rdq, m, 0, 1, rfq, n, 0, 1, bound, match, mismatch, scoreN, go, ge, 2);
      __syncthreads();
      res[0] = fw.score > 65535 ? 65535 : fw.score; res[2] = fw.end_ref; res[4] = ssw_end_read(fw);
      if ((uint32_t)res[0] >= filters && fw.score > 0) {
        const smr::SwRes bw = smr::sw_wave_any_t<false>(rdq, fw.end_read + 1, fw.end_read, -1, rfq, fw.end_ref + 1, fw.end_ref, -1, bound, match, mismatch, scoreN, go, ge, 2);
        __syncthreads();
        res[1] = fw.end_ref - bw.end_ref; res[3] = fw.end_read - bw.end_read;
      }
    }
    if (lane < 5) out[(size_t)pi * 5 + lane] = res[lane];
    __syncthreads();
  }
}

// the same through the four-problems-per-wave kernel (sw_wave_x4): row g of the wave takes pair 4 b + g; forward pass, then the reverse
// pass of the rows whose score passed the filter (the others idle)
__global__ void __launch_bounds__(64) k_ssw_batch_x4(uint32_t n_pairs, const uint8_t* __restrict__ reads, const unsigned long long* __restrict__ read_off,
                                                     const uint8_t* __restrict__ refs, const unsigned long long* __restrict__ ref_off, uint32_t lds_m, uint32_t lds_n,
                                                     int match, int mismatch, int scoreN, int go, int ge, uint32_t filters, int* __restrict__ out) {
  SMR_DYN_LDS(unsigned char, lds_raw);
  const int lane = smr::lane_id(), g = lane >> 4, gl = lane & 15;
  uint8_t* rdq = lds_raw + (size_t)g * lds_m;
  uint8_t* rfq = lds_raw + (size_t)4 * lds_m + (size_t)g * lds_n;
  for (uint32_t p0 = blockIdx.x * 4; p0 < n_pairs; p0 += gridDim.x * 4) {
    const uint32_t pi = p0 + g;
    const bool have = pi < n_pairs;
    int m = have ? (int)(read_off[pi + 1] - read_off[pi]) : 0, n = have ? (int)(ref_off[pi + 1] - ref_off[pi]) : 0;
    if (n == 0) m = 0;
    __syncthreads();
    bool hasn = false;
    for (int q = gl; q < m; q += 16) rdq[q] = reads[read_off[pi] + q];
    for (int q = gl; q < n; q += 16) { const uint8_t ch = refs[ref_off[pi] + q]; rfq[q] = ch; hasn |= ch == 4; }
    __syncthreads();
    int mm = m;
    for (int d = 32; d > 0; d >>= 1) mm = max(mm, __shfl_xor(mm, d, 64));
    const bool hn = __any(hasn);
    int res[5] = {0, -1, -1, -1, m - 1};
    const smr::SwRes fw = smr::sw_wave_x4(rdq, m, 0, 1, rfq, n, 0, 1, match, mismatch, scoreN, go, ge, mm, hn);
    res[0] = fw.score > 65535 ? 65535 : fw.score; res[2] = fw.end_ref; res[4] = m > 0 ? ssw_end_read(fw) : -1;
    const bool rev = m > 0 && (uint32_t)res[0] >= filters && fw.score > 0;
    const smr::SwRes bw = smr::sw_wave_x4(rdq, rev ? fw.end_read + 1 : 0, fw.end_read, -1, rfq, rev ? fw.end_ref + 1 : 0, fw.end_ref, -1, match, mismatch, scoreN, go, ge, mm, hn);
    if (rev) { res[1] = fw.end_ref - bw.end_ref; res[3] = fw.end_read - bw.end_read; }
    if (have && gl < 5) out[(size_t)pi * 5 + gl] = res[gl];
  }
}

extern "C" int smr_ssw_batch(smr_ctx* c, uint32_t n_pairs, const uint8_t* reads, const uint64_t* read_off, const uint8_t* refs, const uint64_t* ref_off,
                             int match, int mismatch, int score_N, int gap_open, int gap_ext, uint32_t filters, int mode, int32_t* out) {
  if (!c || !read_off || !ref_off || !out || mode < 0 || mode > 5) return SMR_ERR_ARG;
  // (modes 0 - 3 are the fast kernels: only under the schemes whose answers they share with ssw.c; mode 4 = the striped slow path, any scheme)
  if (mode != 4) if (const char* why = scheme_unsupported(mismatch, score_N, gap_open, gap_ext)) { set_err(c, why); return SMR_ERR_ARG; }
  if (n_pairs == 0) return SMR_OK;
  (void)hipSetDevice(c->device);
  uint64_t mx_m = 1, mx_n = 1;
  for (uint32_t i = 0; i < n_pairs; i++) { mx_m = std::max(mx_m, read_off[i + 1] - read_off[i]); mx_n = std::max(mx_n, ref_off[i + 1] - ref_off[i]); }
  const uint32_t lm = (uint32_t)((mx_m + 15) & ~15ull), ln = (uint32_t)((mx_n + 15) & ~15ull);
  const size_t lds = (size_t)lm + ln + (size_t)2 * ln * 4;
  if (lds > 60 * 1024) { set_err(c, "smr_ssw_batch: sequences too long for one LDS tile (read + 9 x reference window <= 60 KB)"); return SMR_ERR_CAPACITY; }
  DevPool pool;
  IB_GET(d_reads, uint8_t, read_off[n_pairs] + 1); IB_GET(d_refs, uint8_t, ref_off[n_pairs] + 1);
  IB_GET(d_ro, unsigned long long, (size_t)n_pairs + 1); IB_GET(d_fo, unsigned long long, (size_t)n_pairs + 1);
  IB_GET(d_out, int, (size_t)n_pairs * 5);
  if (read_off[n_pairs]) HIPCHK(c, hipMemcpyAsync(d_reads, reads, read_off[n_pairs], hipMemcpyHostToDevice, c->stream));
  if (ref_off[n_pairs]) HIPCHK(c, hipMemcpyAsync(d_refs, refs, ref_off[n_pairs], hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_ro, read_off, ((size_t)n_pairs + 1) * 8, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_fo, ref_off, ((size_t)n_pairs + 1) * 8, hipMemcpyHostToDevice, c->stream));
  if (mode == 3) {          // four pairs per wave (the kernel k_chain batches candidate windows with): spans up to SW_X4_MAX_ROWS, numbers within the packed range
    for (uint32_t i = 0; i < n_pairs; i++) {
      const uint64_t m = read_off[i + 1] - read_off[i], n = ref_off[i + 1] - ref_off[i];
      if (m > SW_X4_MAX_ROWS || !sw_pk_fits((int)m, (int)n, match, mismatch, score_N, gap_open)) {
        set_err(c, "smr_ssw_batch mode 3: a pair is outside the range of the four-problem kernel"); return SMR_ERR_ARG;
      }
    }
    hipLaunchKernelGGL(k_ssw_batch_x4, dim3(std::min<uint32_t>((n_pairs + 3) / 4, (uint32_t)c->n_cu * 8u)), dim3(64), (size_t)4 * (lm + ln), c->stream, n_pairs, (const uint8_t*)d_reads,
                       (const unsigned long long*)d_ro, (const uint8_t*)d_refs, (const unsigned long long*)d_fo, lm, ln, match, mismatch, score_N, gap_open, gap_ext, filters, d_out);
  } else
  {
    const uint32_t gb = std::min<uint32_t>(n_pairs, (uint32_t)c->n_cu * 8u), stride = 5u * 16u * ((uint32_t)(mx_m + 7) / 8u + 1u);
    uint16_t* d_scr = nullptr;
    if (mode == 4) { IB_GET(d_scr_, uint16_t, (size_t)gb * stride); d_scr = d_scr_; }
    if (mode == 5) hipLaunchKernelGGL(k_ssw_long, dim3(gb), dim3(64), lds, c->stream, n_pairs, (const uint8_t*)d_reads,
                       (const unsigned long long*)d_ro, (const uint8_t*)d_refs, (const unsigned long long*)d_fo, lm, ln, match, mismatch, score_N, gap_open, gap_ext, filters, d_out);
    else if (mode == 4) hipLaunchKernelGGL(k_ssw_batch<true>, dim3(gb), dim3(64), lds, c->stream, n_pairs, (const uint8_t*)d_reads,
                       (const unsigned long long*)d_ro, (const uint8_t*)d_refs, (const unsigned long long*)d_fo, lm, ln, match, mismatch, score_N, gap_open, gap_ext, filters, -1, d_out, d_scr, stride);
    else hipLaunchKernelGGL(k_ssw_batch<false>, dim3(gb), dim3(64), lds, c->stream, n_pairs, (const uint8_t*)d_reads,
                       (const unsigned long long*)d_ro, (const uint8_t*)d_refs, (const unsigned long long*)d_fo, lm, ln, match, mismatch, score_N, gap_open, gap_ext, filters, mode, d_out, d_scr, stride);
  }
  HIPCHK(c, hipMemcpyAsync(out, d_out, (size_t)n_pairs * 5 * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SMR_OK;
}

extern "C" int smr_sw_long_rows(int m) { return smr::sw_long_rows(m); }

// =================================================================================================
// k_sw16 at the same seam: the kernel as the candidate walk launches it (smr_walk.hpp) -- packed records of the selected batch, WTasks, the two
// index lists and the counters as k_walk leaves them -- and, for the tasks scored with end cells, the begin-cell tasks as k_begins_prep makes them.
// =================================================================================================
extern "C" int smr_sw16_batch(smr_ctx* c, uint32_t n_tasks, const smr_sw16_task* tasks, const uint8_t* ref, uint64_t ref_len, int force_any_n,
                              int match, int mismatch, int score_N, int gap_open, int gap_ext, uint32_t filters, int rows, uint32_t blocks, int32_t* out) {
  if (!c || (n_tasks && (!tasks || !out)) || (ref_len && !ref)) return SMR_ERR_ARG;
  if (rows != 13 && rows != 19 && rows != 26 && rows != 32) { set_err(c, "smr_sw16_batch: rows must be 13, 19, 26 or 32"); return SMR_ERR_ARG; }
  if (blocks > 65536u) { set_err(c, "smr_sw16_batch: at most 65536 blocks"); return SMR_ERR_ARG; }
  if (match <= 0 || match > 127 || mismatch > 0 || mismatch < -127 || score_N < -127 || gap_open < 0 || gap_open > 255 || gap_ext < 0 || gap_ext > 255) { set_err(c, "smr_sw16_batch: bad scoring options"); return SMR_ERR_ARG; }
  if (const char* why = scheme_unsupported(mismatch, score_N, gap_open, gap_ext)) { set_err(c, why); return SMR_ERR_ARG; }
  if (!c->b->used || !c->b->d_words) { set_err(c, "smr_sw16_batch: no reads uploaded into the selected batch"); return SMR_ERR_STATE; }
  (void)hipSetDevice(c->device);
  const uint32_t n_reads = c->b->n;
  std::vector<uint32_t> len(n_reads);
  if (n_reads) HIPCHK(c, hipMemcpyAsync(len.data(), c->b->d_len, (size_t)n_reads * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<WTask> tk(std::max<uint32_t>(n_tasks, 1));
  std::vector<uint32_t> ia, ib;
  for (uint32_t i = 0; i < n_tasks; i++) {
    const smr_sw16_task& t = tasks[i];
    const char* why = nullptr;
    if (t.read >= n_reads) why = "read index outside the batch";
    else if (t.m == 0 || t.nref == 0) why = "empty span or window";
    else if (t.m > WK_MAX_ROWS || (int)t.m > 8 * rows) why = "span longer than the kernel takes (8 x rows, at most WK_MAX_ROWS)";
    else if ((uint64_t)t.aq + t.m > len[t.read]) why = "rows outside the read";
    else if ((uint64_t)t.win_off + t.nref > ref_len) why = "window outside the reference letters";
    else if (!sw_pk_fits((int)t.m, (int)t.nref, match, mismatch, score_N, gap_open)) why = "numbers outside the packed representation (sw_pk_fits)";
    else if (t.reversed > 1 || t.list_b > 1) why = "reversed / list_b must be 0 or 1";
    if (why) { set_err(c, std::string("smr_sw16_batch: task ") + std::to_string(i) + ": " + why); return SMR_ERR_ARG; }
    WTask o;
    memset(&o, 0, sizeof o);
    o.r = t.read; o.max_ref = 0; o.rf_start = t.win_off; o.ars = 0; o.head = 0; o.aq = t.aq; o.m = t.m; o.nref = t.nref; o.flags = t.reversed ? 1 : 0;
    tk[i] = o;
    (t.list_b ? ib : ia).push_back(i);
  }
  if (n_tasks == 0) return SMR_OK;
  DevPool pool;
  IB_GET(d_ref, uint8_t, ref_len + 8); IB_GET(d_tk, WTask, n_tasks); IB_GET(d_ia, uint32_t, n_tasks); IB_GET(d_ib, uint32_t, n_tasks);
  IB_GET(d_wc, unsigned long long, WC_STRIDE); IB_GET(d_res, uint2, n_tasks);
  HIPCHK(c, hipMemsetAsync(d_ref, 0, ref_len + 8, c->stream));
  if (ref_len) HIPCHK(c, hipMemcpyAsync(d_ref, ref, ref_len, hipMemcpyHostToDevice, c->stream));
  DIndex ix;
  memset(&ix, 0, sizeof ix);
  ix.ref_seq = d_ref;
  ix.ref_any_n = (force_any_n || (ref_len && memchr(ref, 4, ref_len))) ? 1u : 0u;          // (as smr_index_upload sets it for an index part)
  DParams P;
  memset(&P, 0, sizeof P);
  P.match = match; P.mismatch = mismatch; P.score_N = score_N; P.gap_open = gap_open; P.gap_ext = gap_ext; P.sw_mode = c->sw_mode;
  unsigned long long wc[WC_STRIDE] = {};
  std::vector<uint2> res(n_tasks);
  // forward: list A with end cells, list B score only
  wc[WC_NTASK] = ia.size(); wc[WC_NTASK2] = ib.size();
  HIPCHK(c, hipMemcpyAsync(d_tk, tk.data(), (size_t)n_tasks * sizeof(WTask), hipMemcpyHostToDevice, c->stream));
  if (!ia.empty()) HIPCHK(c, hipMemcpyAsync(d_ia, ia.data(), ia.size() * 4, hipMemcpyHostToDevice, c->stream));
  if (!ib.empty()) HIPCHK(c, hipMemcpyAsync(d_ib, ib.data(), ib.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_wc, wc, sizeof wc, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(d_res, 0xEE, (size_t)n_tasks * sizeof(uint2), c->stream));
  launch_sw16(c, rows, -1, blocks, dreads(c), ix, P, d_tk, d_ia, d_ib, d_ib, d_wc, d_res);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(res.data(), d_res, (size_t)n_tasks * sizeof(uint2), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  // begin cells (k_begins_prep, stage 1): rows back from the end row, columns back from the end column, all in the list with end cells
  std::vector<uint32_t> beg;
  std::vector<WTask> tb(tk);
  for (uint32_t i = 0; i < n_tasks; i++) {
    int32_t* o = out + (size_t)i * 5;
    const int score = res[i].x > 65535u ? 65535 : (int)res[i].x;
    o[0] = score; o[1] = o[2] = o[3] = o[4] = -1;
    if (tasks[i].list_b) {
      if (res[i].y != 0xFFFFFFFFu) { set_err(c, "smr_sw16_batch: a score-only task came back with an end cell"); return SMR_ERR_DEVICE; }
      continue;
    }
    if (res[i].y == 0xFFFFFFFFu || res[i].y == 0xEEEEEEEEu) { set_err(c, "smr_sw16_batch: a task of the end-cell list came back without one"); return SMR_ERR_DEVICE; }
    const int end_ref = (int)(res[i].y >> 16) - 1, end_read = (int)(res[i].y & 0xFFFFu);
    o[2] = end_ref; o[4] = score > 0 ? end_read : 0;          // (no positive cell: ssw_align's read_end1 is 0, see ssw_end_read above)
    // (the second launch reads the read and the window back from this cell: a cell outside the task would send it outside the buffers)
    if (end_ref < -1 || end_ref >= (int)tk[i].nref || end_read >= (int)tk[i].m || (score > 0 && end_ref < 0)) {
      set_err(c, "smr_sw16_batch: task " + std::to_string(i) + " came back with an end cell outside its span and window"); return SMR_ERR_DEVICE;
    }
    if ((uint32_t)score >= filters && score > 0) {
      WTask& b = tb[i];
      b.m = (uint16_t)(end_read + 1); b.nref = (uint16_t)(end_ref + 1);
      b.aq = (uint16_t)(tk[i].aq + end_read); b.rf_start = tk[i].rf_start + (uint64_t)end_ref; b.flags = (uint16_t)(tk[i].flags | 2u);
      beg.push_back(i);
    }
  }
  if (beg.empty()) return SMR_OK;
  memset(wc, 0, sizeof wc);
  wc[WC_NTASK] = beg.size();
  HIPCHK(c, hipMemcpyAsync(d_tk, tb.data(), (size_t)n_tasks * sizeof(WTask), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_ia, beg.data(), beg.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_wc, wc, sizeof wc, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(d_res, 0xEE, (size_t)n_tasks * sizeof(uint2), c->stream));
  launch_sw16(c, rows, -1, blocks, dreads(c), ix, P, d_tk, d_ia, d_ib, d_ib, d_wc, d_res);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(res.data(), d_res, (size_t)n_tasks * sizeof(uint2), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (uint32_t i : beg) {
    int32_t* o = out + (size_t)i * 5;
    if (res[i].y == 0xFFFFFFFFu || res[i].y == 0xEEEEEEEEu) { set_err(c, "smr_sw16_batch: a begin-cell task came back without a cell"); return SMR_ERR_DEVICE; }
    const int b_ref = (int)(res[i].y >> 16) - 1, b_read = (int)(res[i].y & 0xFFFFu);
    o[1] = o[2] - b_ref; o[3] = o[4] - b_read;
  }
  return SMR_OK;
}

// the prefix tasks of k_sw16 at the same seam: all tasks in the third list, each over the first `cols` columns of its window
extern "C" int smr_sw16_prefix_batch(smr_ctx* c, uint32_t n_tasks, const smr_sw16_prefix_task* tasks, const uint8_t* ref, uint64_t ref_len, int force_any_n,
                                     int match, int mismatch, int score_N, int gap_open, int gap_ext, int rows, uint32_t blocks, int32_t* out) {
  if (!c || (n_tasks && (!tasks || !out)) || (ref_len && !ref)) return SMR_ERR_ARG;
  if (rows != 13 && rows != 19 && rows != 26 && rows != 32) { set_err(c, "smr_sw16_prefix_batch: rows must be 13, 19, 26 or 32"); return SMR_ERR_ARG; }
  if (blocks > 65536u) { set_err(c, "smr_sw16_prefix_batch: at most 65536 blocks"); return SMR_ERR_ARG; }
  if (match <= 0 || match > 127 || mismatch > 0 || mismatch < -127 || score_N < -127 || gap_open < 0 || gap_open > 255 || gap_ext < 0 || gap_ext > 255) { set_err(c, "smr_sw16_prefix_batch: bad scoring options"); return SMR_ERR_ARG; }
  if (const char* why = scheme_unsupported(mismatch, score_N, gap_open, gap_ext)) { set_err(c, why); return SMR_ERR_ARG; }
  if (!c->b->used || !c->b->d_words) { set_err(c, "smr_sw16_prefix_batch: no reads uploaded into the selected batch"); return SMR_ERR_STATE; }
  (void)hipSetDevice(c->device);
  const uint32_t n_reads = c->b->n;
  std::vector<uint32_t> len(n_reads);
  if (n_reads) HIPCHK(c, hipMemcpyAsync(len.data(), c->b->d_len, (size_t)n_reads * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  std::vector<WTask> tk(std::max<uint32_t>(n_tasks, 1));
  std::vector<uint32_t> ic(std::max<uint32_t>(n_tasks, 1));
  for (uint32_t i = 0; i < n_tasks; i++) {
    const smr_sw16_prefix_task& t = tasks[i];
    const char* why = nullptr;
    if (t.read >= n_reads) why = "read index outside the batch";
    else if (t.m == 0 || t.nref == 0) why = "empty span or window";
    else if (t.m > WK_MAX_ROWS || (int)t.m > 8 * rows) why = "span longer than the kernel takes (8 x rows, at most WK_MAX_ROWS)";
    else if ((uint64_t)t.aq + t.m > len[t.read]) why = "rows outside the read";
    else if ((uint64_t)t.win_off + t.nref > ref_len) why = "window outside the reference letters";
    else if (!sw_pk_fits((int)t.m, (int)t.nref, match, mismatch, score_N, gap_open)) why = "numbers outside the packed representation (sw_pk_fits)";
    else if (t.reversed > 1) why = "reversed must be 0 or 1";
    else if (t.cols == 0) why = "cols must not be 0";
    else if (t.cols % 4u) why = "cols must be a multiple of 4 (the kernel's period)";
    else if (t.cols >= t.nref) why = "cols must be less than nref";
    if (why) { set_err(c, std::string("smr_sw16_prefix_batch: task ") + std::to_string(i) + ": " + why); return SMR_ERR_ARG; }
    WTask o;
    memset(&o, 0, sizeof o);
    o.r = t.read; o.rf_start = t.win_off; o.aq = t.aq; o.m = t.m; o.nref = t.nref; o.flags = (uint16_t)((t.reversed ? 1u : 0u) | t.cols);
    tk[i] = o; ic[i] = i;
  }
  if (n_tasks == 0) return SMR_OK;
  DevPool pool;
  IB_GET(d_ref, uint8_t, ref_len + 8); IB_GET(d_tk, WTask, n_tasks); IB_GET(d_ic, uint32_t, n_tasks);
  IB_GET(d_wc, unsigned long long, WC_STRIDE); IB_GET(d_res, uint2, n_tasks);
  HIPCHK(c, hipMemsetAsync(d_ref, 0, ref_len + 8, c->stream));
  if (ref_len) HIPCHK(c, hipMemcpyAsync(d_ref, ref, ref_len, hipMemcpyHostToDevice, c->stream));
  DIndex ix;
  memset(&ix, 0, sizeof ix);
  ix.ref_seq = d_ref;
  ix.ref_any_n = (force_any_n || (ref_len && memchr(ref, 4, ref_len))) ? 1u : 0u;
  DParams P;
  memset(&P, 0, sizeof P);
  P.match = match; P.mismatch = mismatch; P.score_N = score_N; P.gap_open = gap_open; P.gap_ext = gap_ext; P.sw_mode = c->sw_mode;
  unsigned long long wc[WC_STRIDE] = {};
  std::vector<uint2> res(n_tasks);
  wc[WC_NTASK3] = n_tasks;
  HIPCHK(c, hipMemcpyAsync(d_tk, tk.data(), (size_t)n_tasks * sizeof(WTask), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_ic, ic.data(), (size_t)n_tasks * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_wc, wc, sizeof wc, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemsetAsync(d_res, 0xEE, (size_t)n_tasks * sizeof(uint2), c->stream));
  launch_sw16(c, rows, -1, blocks, dreads(c), ix, P, d_tk, d_ic, d_ic, d_ic, d_wc, d_res);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(res.data(), d_res, (size_t)n_tasks * sizeof(uint2), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (uint32_t i = 0; i < n_tasks; i++) {
    if (res[i].y != WRES_PREFIX) { set_err(c, "smr_sw16_prefix_batch: a prefix task came back without an interval"); return SMR_ERR_DEVICE; }
    out[2 * (size_t)i] = (int32_t)(res[i].x & 0xFFFFu); out[2 * (size_t)i + 1] = (int32_t)(res[i].x >> 16);
  }
  return SMR_OK;
}

// prefix tasks of the candidate walk since smr_prof_reset: out[0] left for k_sw16, [1] consumed decisively, [2] met undecided (left again in full),
// [3] never looked at, [4] / [5] look-ahead tasks of reads expected to align under best N (whatever the mode) and their cells, [6] SMR_WALK_PREFIX as latched,
// [7] 1 while the context leaves prefix tasks, 0 after a part whose intervals mostly stayed undecided (adapt_walk_prefix)
extern "C" int smr_walk_prefix_stats(smr_ctx* c, uint64_t out[8]) {
  if (!c || !out) return SMR_ERR_ARG;
  unsigned long long h[WPS_N] = {};
  if (c->d_wpstat) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(h, c->d_wpstat, sizeof h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  out[0] = h[WPS_SCORED]; out[1] = h[WPS_DECIDED]; out[2] = h[WPS_REDONE]; out[3] = h[WPS_SCORED] - h[WPS_DECIDED] - h[WPS_REDONE];
  out[4] = h[WPS_AHEAD]; out[5] = h[WPS_AHEAD_CELLS]; out[6] = c->tune.walk_prefix; out[7] = c->pfx_live ? 1 : 0;
  return SMR_OK;
}

extern "C" int smr_sw16_launches(const smr_ctx* c, uint64_t out[8]) {
  if (!c || !out) return SMR_ERR_ARG;
  for (int k = 0; k < 8; k++) out[k] = c->sw16_launches[k];
  return SMR_OK;
}

// k_sw16h against k_sw16 on the device (smr_create): for each of the four instantiations, seeded pseudo-random reads (~1.5 % N) of 1 .. 8 R letters
// against a mutated copy between random flanks (3 of 4) or an unrelated window, each as a task with end cells (every fourth one a begin-cell
// task, rows and columns backwards), as a score-only task and, where the window has more than four columns, as a prefix task; the two
// scoring schemes of smr_sw_selfcheck in turn.  *n_bad: results (8 bytes each) on which the kernels differ.
int sw16h_selfcheck(smr_ctx* c, uint32_t cases, uint32_t seed, uint64_t* n_bad) {
  *n_bad = 0;
  const uint32_t n_reads = std::min<uint32_t>(cases, 64u);
  if (n_reads == 0) return SMR_OK;
  static const int ROWS[4] = {13, 19, 26, 32};
  static const int SC[2][3] = {{2, -3, -3}, {5, -4, -4}};
  uint32_t x = seed | 1u;
  auto rnd = [&x]() { x ^= x << 13; x ^= x >> 17; x ^= x << 5; return x >> 8; };
  DevPool pool;
  for (int v = 0; v < 4; v++) {
    const uint32_t max_m = std::min<uint32_t>(8u * (uint32_t)ROWS[v], WK_MAX_ROWS);
    std::vector<uint32_t> words, len(n_reads);
    std::vector<uint64_t> rec_off(n_reads);
    std::vector<uint8_t> ref;
    std::vector<WTask> tk;
    std::vector<uint32_t> ia, ib, ic;
    for (uint32_t r = 0; r < n_reads; r++) {
      const uint32_t m = r == 0 ? max_m : 1u + rnd() % max_m;
      std::vector<uint8_t> rd(m);
      for (auto& ch : rd) { const uint32_t h = rnd(); ch = (h & 63u) == 0 ? 4 : (uint8_t)((h >> 8) & 3u); }
      len[r] = m; rec_off[r] = words.size();
      const size_t cw = (m + 15u) >> 4, aw = (m + 31u) >> 5, w0 = words.size();
      words.resize(w0 + cw + aw, 0u);
      for (uint32_t q = 0; q < m; q++) {
        if (rd[q] == 4) words[w0 + cw + (q >> 5)] |= 1u << (q & 31);
        else words[w0 + (q >> 4)] |= (uint32_t)rd[q] << ((q & 15) * 2);
      }
      const uint32_t hm = rnd();
      const bool homolog = (hm & 3u) != 0, reversed = (hm >> 2) & 1u;
      const uint64_t win_off = ref.size();
      for (uint32_t q = 0, fl = (hm >> 4) & 15u; q < fl; q++) ref.push_back((uint8_t)(rnd() & 3u));
      for (uint32_t q = 0; q < m; q++) {
        // (a forward read's letters as they are; a reversed one is read complemented from its end, so its homolog is the reverse complement)
        const uint8_t own = reversed ? (rd[m - 1 - q] == 4 ? 0 : (uint8_t)(3 - rd[m - 1 - q])) : (rd[q] == 4 ? 0 : rd[q]);
        const uint32_t h = rnd(), ev = (h >> 4) & 63u;
        if (!homolog) { ref.push_back((uint8_t)(h & 3u)); continue; }
        if (ev == 0) continue;
        if (ev == 1) ref.push_back((uint8_t)((h >> 12) & 3u));
        if (ev == 2) { ref.push_back(4); continue; }
        ref.push_back(ev < 6 ? (uint8_t)((h >> 16) & 3u) : own);
      }
      for (uint32_t q = 0, fl = (hm >> 8) & 15u; q < fl; q++) ref.push_back((uint8_t)(rnd() & 3u));
      if (ref.size() == win_off) ref.push_back(0);
      const uint32_t nref = (uint32_t)(ref.size() - win_off);
      WTask t;
      memset(&t, 0, sizeof t);
      t.r = r; t.rf_start = win_off; t.aq = 0; t.m = (uint16_t)m; t.nref = (uint16_t)nref; t.flags = reversed ? 1 : 0;
      WTask ta = t;
      if ((r & 3u) == 3u) { ta.aq = (uint16_t)(m - 1); ta.rf_start = win_off + nref - 1; ta.flags |= 2u; }
      ia.push_back((uint32_t)tk.size()); tk.push_back(ta);
      ib.push_back((uint32_t)tk.size()); tk.push_back(t);
      if (nref > 4) {
        WTask tc = t;
        tc.flags |= (uint16_t)(4u * (1u + rnd() % ((nref - 1u) / 4u)));      // cols: a multiple of 4 in [4, nref)
        ic.push_back((uint32_t)tk.size()); tk.push_back(tc);
      }
    }
    words.resize(words.size() + 4, 0u);          // (the kernel's 12-byte and 8-byte loads may begin in a record's last word)
    const uint32_t n_tasks = (uint32_t)tk.size();
    IB_GET(d_words, uint32_t, words.size()); IB_GET(d_off, uint64_t, n_reads); IB_GET(d_len, uint32_t, n_reads);
    IB_GET(d_ref, uint8_t, ref.size() + 8); IB_GET(d_tk, WTask, n_tasks);
    IB_GET(d_ia, uint32_t, n_tasks); IB_GET(d_ib, uint32_t, n_tasks); IB_GET(d_ic, uint32_t, n_tasks);
    IB_GET(d_wc, unsigned long long, WC_STRIDE); IB_GET(d_res, uint2, (size_t)2 * n_tasks);
    HIPCHK(c, hipMemcpyAsync(d_words, words.data(), words.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_off, rec_off.data(), (size_t)n_reads * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_len, len.data(), (size_t)n_reads * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_ref, 0, ref.size() + 8, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_ref, ref.data(), ref.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_tk, tk.data(), (size_t)n_tasks * sizeof(WTask), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_ia, ia.data(), ia.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_ib, ib.data(), ib.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!ic.empty()) HIPCHK(c, hipMemcpyAsync(d_ic, ic.data(), ic.size() * 4, hipMemcpyHostToDevice, c->stream));
    unsigned long long wc[WC_STRIDE] = {};
    wc[WC_NTASK] = ia.size(); wc[WC_NTASK2] = ib.size(); wc[WC_NTASK3] = ic.size();
    HIPCHK(c, hipMemcpyAsync(d_wc, wc, sizeof wc, hipMemcpyHostToDevice, c->stream));
    DReads rd;
    rd.words = d_words; rd.rec_off = d_off; rd.len = d_len; rd.n = n_reads; rd.max_len = max_m;
    DIndex ix;
    memset(&ix, 0, sizeof ix);
    ix.ref_seq = d_ref; ix.ref_any_n = 1u;
    std::vector<uint2> res((size_t)2 * n_tasks);
    for (int k = 0; k < 2; k++) {
      DParams P;
      memset(&P, 0, sizeof P);
      P.match = SC[k][0]; P.mismatch = SC[k][1]; P.score_N = SC[k][2]; P.gap_open = 5; P.gap_ext = 2; P.sw_mode = c->sw_mode;
      if (!sw_h16_fits((int)max_m, P.match, P.mismatch, P.score_N, P.gap_open, P.gap_ext)) continue;
      HIPCHK(c, hipMemsetAsync(d_res, 0xEE, (size_t)2 * n_tasks * sizeof(uint2), c->stream));
      launch_sw16(c, ROWS[v], -1, 0, rd, ix, P, d_tk, d_ia, d_ib, d_ic, d_wc, d_res, 0);
      launch_sw16(c, ROWS[v], -1, 0, rd, ix, P, d_tk, d_ia, d_ib, d_ic, d_wc, d_res + n_tasks, 1);
      HIPCHK(c, hipGetLastError());
      HIPCHK(c, hipMemcpyAsync(res.data(), d_res, (size_t)2 * n_tasks * sizeof(uint2), hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      for (uint32_t i = 0; i < n_tasks; i++) {
        const uint2 a = res[i], b = res[(size_t)n_tasks + i];
        if (a.x != b.x || a.y != b.y || (a.x == 0xEEEEEEEEu && a.y == 0xEEEEEEEEu)) (*n_bad)++;
      }
    }
  }
  return SMR_OK;
}

// k_sw16h, the packed-f16 flavour of k_sw16: set_to 0 / 1 = select, anything else = query only; returns the mode in use (0 too after a failed self-check
// of smr_create or under SMR_SW16_F16=0).  launches (may be null): k_sw16h<R> launched since smr_create, whoever asked for them.
extern "C" int smr_sw16_f16(smr_ctx* c, int set_to, uint64_t* launches) {
  if (!c) return SMR_ERR_ARG;
  if (set_to == 0 || set_to == 1) c->sw16_f16 = set_to;
  if (launches) *launches = c->sw16h_launches;
  return c->sw16_f16;
}

extern "C" int smr_sw_mode(smr_ctx* c, int set_to) {      // set_to: 0 / 1 = select, anything else = query only; returns the mode in use
  if (!c) return SMR_ERR_ARG;
  if (set_to >= 0 && set_to <= 2) c->sw_mode = set_to;
  return c->sw_mode;
}

// rounds the candidate walk of the next part runs per pass (smr_walk.hpp; adapts to what the previous part needed unless SMR_WALK_ROUNDS fixes it)
extern "C" int smr_walk_rounds(const smr_ctx* c, uint32_t out[3]) {
  if (!c || !out) return SMR_ERR_ARG;
  for (int p = 0; p < 3; p++) out[p] = (!c->tune.walk_rounds_fixed && c->walk_need[p]) ? std::min(c->tune.walk_rounds, c->walk_need[p]) : c->tune.walk_rounds;
  return SMR_OK;
}
