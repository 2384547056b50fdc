// smr_engine_chain.hpp -- host side of the candidate stage (included by smr_engine.hip inside its anonymous namespace): LDS budgets, scratch of the long-read strips,
// the rounds of the candidate walk and how their number adapts, launch_chain.
// (one translation unit: no include guard games -- this file is text of smr_engine.hip, cut out along its stages)

uint32_t chain_edges(const DParams& P, uint32_t len) { return P.is_as_percent ? (uint32_t)((P.edges / 100.0) * len) + 1 : (uint32_t)std::max(P.edges, 0); }
// ml / rf: the longest read / reference window of the batch (rounded to 16); rq: the longest window of a read of <= SW_X4_MAX_ROWS letters
void chain_lds(const smr_ctx* c, const DParams& P, uint32_t& ml, uint32_t& rf, uint32_t& rq, size_t& bytes) {
  const uint32_t mq_len = std::min<uint32_t>(c->b->max_len, SW_X4_MAX_ROWS);
  ml = (c->b->max_len + 15) & ~15u;
  rf = (c->b->max_len + 2 * chain_edges(P, c->b->max_len) + 16 + 15) & ~15u;
  rq = std::min(rf, (mq_len + 2 * chain_edges(P, mq_len) + 16 + 15) & ~15u);
  bytes = 5 * (size_t)std::min<uint32_t>(ml, SW_X4_MAX_ROWS) + (size_t)9 * rq + (size_t)CH_KEYS_LDS * 8 + (size_t)std::max<uint32_t>(4u * CH_PAIRS_LDS, 2u * c->chain_scap) * 4 +
          (size_t)CH_HITS_LDS * 8 + (size_t)(CH_HITS_LDS + 8) * 4 + (size_t)c->chain_scap * 4;
}
void chain_lds(const smr_ctx* c, const DParams& P, uint32_t& ml, uint32_t& rf, size_t& bytes) { uint32_t rq; chain_lds(c, P, ml, rf, rq, bytes); }
// per block: strip-boundary rows of the Smith-Waterman kernels (2 ints per reference column) and the letters of the read being walked
// (1 byte each) -- only batches with reads of more than one strip
int ensure_bound(smr_ctx* c, uint32_t blocks, uint32_t rf) {
  if (c->b->max_len <= SW_X4_MAX_ROWS) return SMR_OK;
  int rc = c->d_bound.reserve(c, (size_t)blocks * 2 * rf);
  return rc ? rc : c->d_rdq.reserve(c, (size_t)blocks * ((c->b->max_len + 15) & ~15u));
}

// What one smr_align_part settles once for all its launches.  lng: the batch has reads of more than one Smith-Waterman strip (the short-read
// instantiations carry none of their state).  striped: the slow path that reproduces ssw.c's stripe geometry (instantiations of its own); it
// scores in k_chain and k_begins alone, so neither the candidate walk in rounds (split) nor four problems per wave (x4) go with it -- both
// want the packed kernels.  begins_sw16: the begin cells sixteen per wave through k_sw16 (launch_begins adds only whether the walk's task
// buffers are there and large enough).  rows: the k_sw16 instantiation for the batch's spans.
struct AlignPlan { uint32_t ml, rf, rq; size_t lds; bool lng, striped, split, x4, begins_sw16; int rows; };
int sw16_rows(uint32_t max_len) {
  const uint32_t wmq = std::min<uint32_t>(max_len, WK_MAX_ROWS);
  return wmq <= 104 ? 13 : wmq <= 152 ? 19 : wmq <= 208 ? 26 : 32;
}
AlignPlan align_plan(const smr_ctx* c, const DParams& P) {
  AlignPlan a;
  chain_lds(c, P, a.ml, a.rf, a.rq, a.lds);
  const uint32_t max_len = c->b->max_len;
  const bool packed = P.sw_mode >= 1;
  a.lng = max_len > SW_X4_MAX_ROWS;
  a.striped = P.sw_mode < 0;
  // the split path takes the marked reads with a record of k_cand (the hand-over) whose Smith-Waterman problems fit the packed kernels
  a.split = packed && c->tune.walk_split && c->tune.handover && sw_pk_fits((int)std::min<uint32_t>(max_len, WK_MAX_ROWS), (int)a.rq, P.match, P.mismatch, P.score_N, P.gap_open);
  a.x4 = packed && !a.lng && sw_pk_fits((int)max_len, (int)a.rf, P.match, P.mismatch, P.score_N, P.gap_open);
  a.begins_sw16 = a.x4 && c->tune.walk_split && !c->tune.begins_x4;
  a.rows = sw16_rows(max_len);
  return a;
}

// the instantiation of each kernel family for the flags that select it (all of them: what raise_lds_limit is given)
typedef decltype(&k_chain<false, false, false>) chain_fn;
chain_fn chain_kernel(bool ext, bool lng, bool striped) {
  static const chain_fn K[8] = {k_chain<false, false, false>, k_chain<true, false, false>, k_chain<false, true, false>, k_chain<true, true, false>,
                                k_chain<false, false, true>,  k_chain<true, false, true>,  k_chain<false, true, true>,  k_chain<true, true, true>};
  return K[(ext ? 1 : 0) | (lng ? 2 : 0) | (striped ? 4 : 0)];
}
typedef decltype(&k_begins<false, false>) begins_fn;
begins_fn begins_kernel(bool lng, bool striped) {
  static const begins_fn K[4] = {k_begins<false, false>, k_begins<true, false>, k_begins<false, true>, k_begins<true, true>};
  return K[(lng ? 1 : 0) | (striped ? 2 : 0)];
}
// k_sw16<rows> or k_sw16h<rows> over one task list (smr_walk.hpp).  counted: 0 = a walk round, 4 = the begin-cell stage (smr_sw16_launches), < 0 = not counted (the
// test seam); blocks 0: what fills the device
typedef decltype(&k_sw16<13>) sw16_fn;
void launch_sw16(smr_ctx* c, int rows, int counted, uint32_t blocks, const DReads& rd, const DIndex& ix, const DParams& P, const WTask* tasks, const uint32_t* tix, const uint32_t* tix2,
                 const uint32_t* tix3, const unsigned long long* wc, uint2* res, int flavour = -1) {      // flavour: -1 = the dispatcher's choice, 0 / 1 = k_sw16 / k_sw16h (the self-check of smr_create)
  static const sw16_fn K[2][4] = {{k_sw16<13>, k_sw16<19>, k_sw16<26>, k_sw16<32>}, {k_sw16h<13>, k_sw16h<19>, k_sw16h<26>, k_sw16h<32>}};
  const int v = rows == 13 ? 0 : rows == 19 ? 1 : rows == 26 ? 2 : 3;
  // the f16 flavour (three-operand maxima) where the scheme and the longest span of this instantiation stay within what f16 holds exactly
  const int h = (flavour < 0 ? c->sw16_f16 != 0 : flavour == 1) && sw_h16_fits(std::min<int>(8 * rows, (int)WK_MAX_ROWS), P.match, P.mismatch, P.score_N, P.gap_open, P.gap_ext) ? 1 : 0;
  c->sw16h_launches += (uint64_t)h;
  launch(c, K[h][v], dim3(blocks ? blocks : (uint32_t)c->n_cu * 4u * (uint32_t)SW16_WAVES(rows)), dim3(64), 0, rd, ix, P, tasks, tix, tix2, tix3, wc, res);
  if (counted >= 0) c->sw16_launches[counted + v]++;
}

__global__ void k_wstat(const unsigned long long* __restrict__ wctr, unsigned long long* __restrict__ out, uint32_t rounds) {
  if (threadIdx.x < 32) out[threadIdx.x] = threadIdx.x < rounds ? wctr[(size_t)threadIdx.x * WC_STRIDE + WC_NLIST] : 0ull;
}
// After a part (the stream is idle): how many rounds its (strand, pass) launches needed -- the last round that listed more reads than the
// closing round takes in its stride, + that closing round; when the closing round itself was that full, two more next time.  Whatever the
// number, the closing round ends every listed read's pass: the records do not depend on it (WALK_VARIANTS of the parity tests).
int adapt_walk_rounds(smr_ctx* c) {
  if (c->tune.walk_rounds_fixed || !c->wstat_n || !c->d_wstat) return SMR_OK;
  unsigned long long h[8 * 32];
  HIPCHK(c, hipMemcpyAsync(h, c->d_wstat, (size_t)c->wstat_n * 32 * 8, hipMemcpyDeviceToHost, c->stream));       // (on the context's stream, like read_ctr: no other stream is waited for)
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const unsigned long long few = (unsigned long long)c->n_cu * 8ull;
  uint32_t need[3] = {0, 0, 0};
  for (uint32_t e = 0; e < c->wstat_n; e++) {
    uint32_t want = 2;
    for (uint32_t r = 0; r < c->wstat_rm[e]; r++) if (h[e * 32 + r] > few) want = r + 2 + (r + 1 == c->wstat_rm[e] ? 2u : 0u);
    need[c->wstat_pass[e]] = std::max(need[c->wstat_pass[e]], want);
  }
  // more rounds at once; fewer by half the difference per part (parts of one run differ: eight databases, batches of a mixed sample)
  for (int p = 0; p < 3; p++) if (need[p]) {
    const uint32_t prev = c->walk_need[p] ? c->walk_need[p] : c->tune.walk_rounds;
    c->walk_need[p] = std::min(c->tune.walk_rounds, need[p] >= prev ? need[p] : prev - std::max(1u, (prev - need[p]) / 2u));
  }
  c->wstat_n = 0;
  return SMR_OK;
}

// After a part (the stream is idle): did its prefix tasks pay?  An undecided interval is a window scored twice and a read listed for one more round,
// so data whose scores lie close together (real amplicon reads against references clustered at 95 % identity) loses by the mode what families of
// distant members win.  The context stops leaving prefix tasks when a part met fewer than two decided intervals per undecided one, and tries
// again WALK_PREFIX_RETRY parts later (the parts of a run differ: eight databases, batches of a mixed sample).  Only which windows are scored
// over a prefix depends on it, never a record.
#define WALK_PREFIX_RETRY 64u
#define WALK_PREFIX_MIN_SEEN 64ull                       // intervals consumed in a part before it says anything
int adapt_walk_prefix(smr_ctx* c) {
  if (!c->tune.walk_prefix || !c->d_wpstat) return SMR_OK;
  if (!c->pfx_live) { if (++c->pfx_parts_off >= WALK_PREFIX_RETRY) { c->pfx_live = true; c->pfx_parts_off = 0; } return SMR_OK; }
  unsigned long long h[WPS_N];
  HIPCHK(c, hipMemcpyAsync(h, c->d_wpstat, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (h[WPS_DECIDED] < c->pfx_seen[0] || h[WPS_REDONE] < c->pfx_seen[1]) c->pfx_seen[0] = c->pfx_seen[1] = 0;      // (smr_prof_reset in between)
  const unsigned long long dec = h[WPS_DECIDED] - c->pfx_seen[0], redo = h[WPS_REDONE] - c->pfx_seen[1];
  c->pfx_seen[0] = h[WPS_DECIDED]; c->pfx_seen[1] = h[WPS_REDONE];
  if (dec + redo >= WALK_PREFIX_MIN_SEEN && dec < 2 * redo) {
    c->pfx_live = false; c->pfx_parts_off = 0;
    say(c->tune, "prefix tasks off for %u parts: %llu intervals decided, %llu undecided in the last part\n", WALK_PREFIX_RETRY, dec, redo);
  }
  return SMR_OK;
}

int launch_chain(smr_ctx* c, const DevIndex& di, const DParams& P, const AlignPlan& plan, int pass, int is_last_strand) {
  Batch& B = *c->b;
  const uint32_t ml = plan.ml, rf = plan.rf, rq = plan.rq;
  const size_t lds = plan.lds;
  const bool split = plan.split;
  int rc;
  HIPCHK(c, hipMemsetAsync(&B.d_ctr[C_WORK_NEXT], 0, 8, c->stream));
  // reads beyond ~5.6 kb: more than the default 64 KB of dynamic LDS per workgroup (gfx950 has 160 KB per CU)
  if ((rc = raise_lds_limit(c, c->chain_lds_attr, lds, 64 * 1024, chain_kernel(0, 0, 0), chain_kernel(1, 0, 0), chain_kernel(0, 1, 0), chain_kernel(1, 1, 0),
                            chain_kernel(0, 0, 1), chain_kernel(1, 0, 1), chain_kernel(0, 1, 1), chain_kernel(1, 1, 1)))) return rc;
  const uint32_t blocks = std::min<uint32_t>(c->chain_blocks, std::max(B.n, 1u));
  if ((rc = ensure_bound(c, c->chain_blocks, rf))) return rc;
  int* const gb = plan.lng ? c->d_bound.get() : nullptr;
  uint8_t* const grd = plan.lng ? c->d_rdq.get() : nullptr;
  if (c->tune.handover) {
    // {offset, npos} per read; CAND_REC_WORDS words per read of the batch, one slice per block of k_cand
    if ((rc = c->d_mrec.reserve(c, B.n)) || (rc = c->d_mpool.reserve(c, (size_t)((B.n + CAND_BLOCK - 1u) / CAND_BLOCK) * CAND_BLOCK * CAND_REC_WORDS))) return rc;
  }
  const uint2* const mrec = c->tune.handover ? c->d_mrec.get() : nullptr;
  const uint32_t wml = (std::min<uint32_t>(B.max_len, WK_MAX_ROWS) + 15) & ~15u;
  const uint32_t RMX = c->tune.walk_rounds, WK = c->tune.walk_k;         // RMX: what d_wctr is laid out for; RM: the rounds of this launch
  const uint32_t RM = (!c->tune.walk_rounds_fixed && c->walk_need[pass]) ? std::min(RMX, c->walk_need[pass]) : RMX;
  if (split) {
    const size_t n = B.n;
    if (c->walk_cap < n || c->walk_kcap < WK) {
      for (int q = 0; q < 2; q++)
        if ((rc = c->d_wlist[q].alloc(c, n)) || (rc = c->d_wstate[q].alloc(c, n)) || (rc = c->d_wtask[q].alloc(c, n * WK)) || (rc = c->d_wres[q].alloc(c, n * WK))) return rc;
      if ((rc = c->d_wtidx.alloc(c, 3 * n * WK)) || (rc = c->d_wslow.alloc(c, n))) return rc;
      c->walk_cap = n; c->walk_kcap = WK;
    }
    if ((rc = c->d_wctr.reserve(c, (size_t)(RMX + 2) * WC_STRIDE)) || (rc = c->d_wstat.reserve(c, (size_t)8 * 32))) return rc;      // (RMX is the context's: made once)
    HIPCHK(c, hipMemsetAsync(c->d_wctr, 0, (size_t)(RMX + 2) * WC_STRIDE * 8, c->stream));
    if (!c->d_wpstat) { if ((rc = c->d_wpstat.alloc(c, WPS_N))) return rc; HIPCHK(c, hipMemsetAsync(c->d_wpstat, 0, WPS_N * 8, c->stream)); }
    if ((rc = raise_lds_limit(c, c->walk_lds_attr, (size_t)wml + rq, 64 * 1024, k_walk<true>))) return rc;
  }
  const size_t n_tix = (size_t)c->walk_cap * c->walk_kcap;     // the second third of d_wtidx: the score-only tasks, the last third: the prefix tasks
  unsigned long long* const n_slow = split ? c->d_wctr + (size_t)(RMX + 1) * WC_STRIDE : nullptr;
  const dim3 per_read((B.n + 255u) / 256u);
  ev_mark(c, KP_CAND);
  // the reads without any candidate reference end their pass in k_cand; k_chain walks the ones it marks
  launch(c, k_cand, dim3((B.n + CAND_BLOCK - 1u) / CAND_BLOCK), dim3(256), CAND_LDS_BYTES(c->cand_bloom, c->tune.handover), dreads(c), dindex(di), P, pass, is_last_strand, B.d_work, B.d_rw, c->d_pool, B.d_marks, c->cand_bloom,
         c->tune.handover ? c->d_mrec.get() : nullptr, c->d_mpool, c->d_mpool.cap());
  if (split) {
    // rounds of walk -> Smith-Waterman -> next list (smr_walk.hpp); the last round scores in the walk kernel, so every listed read ends its pass here
    ev_mark(c, KP_WNEXT);
    launch(c, k_wlist, dim3((B.n + 1023u) / 1024u), dim3(1024), 0, dreads(c), B.d_marks, mrec, (uint32_t)WK_MAX_ROWS, c->d_wlist[0], c->d_wslow, c->d_wctr, n_slow, c->tune.walk_debug ? n_slow + 8 : nullptr, (P.num_seeds >= 2 && c->tune.walk_gather) ? 1 : 0);
    if (c->cinfo_on) launch(c, k_cand_route, per_read, dim3(256), 0, B.n, B.d_marks, mrec, c->d_wlist[0], c->d_wctr, 0, c->d_croute);
    const uint32_t walk_blocks = (uint32_t)c->n_cu * 4u * SMR_WALK_WAVES_PER_SIMD;
    for (uint32_t rnd = 0; rnd < RM; rnd++) {
      const int cur = (int)(rnd & 1u), prv = cur ^ 1;
      unsigned long long* const wc = c->d_wctr + (size_t)rnd * WC_STRIDE;
      const bool fin = rnd + 1 == RM;
      ev_mark(c, KP_WALK);
      launch(c, fin ? k_walk<true> : k_walk<false>, dim3(fin ? walk_blocks * 3u / SMR_WALK_WAVES_PER_SIMD : walk_blocks), dim3(64), fin ? (size_t)wml + rq : 0,
             dreads(c), dindex(di), P, pass, is_last_strand, B.d_work, B.d_work_aln, B.d_rw, B.d_ctr, mrec, c->d_mpool, c->d_pool, c->d_wlist[cur],
             c->d_wstate[prv], c->d_wtask[prv], c->d_wres[prv], c->d_wstate[cur], c->d_wtask[cur], c->d_wtidx, c->d_wtidx + n_tix, c->d_wtidx + 2 * n_tix, wc, WK, n_tix, (int)rnd, wml, rq, c->tune.walk_assume,
             c->pfx_live ? c->tune.walk_prefix : 0u, c->d_wpstat);
      if (fin) continue;
      ev_mark(c, KP_SW16);
      launch_sw16(c, plan.rows, 0, 0, dreads(c), dindex(di), P, c->d_wtask[cur], c->d_wtidx, c->d_wtidx + n_tix, c->d_wtidx + 2 * n_tix, wc, c->d_wres[cur]);
      ev_mark(c, KP_WNEXT);
      launch(c, k_wnext, dim3((uint32_t)c->n_cu * 2u), dim3(1024), 0, P, is_last_strand, B.d_work, B.d_rw, B.d_ctr, c->d_wlist[cur], c->d_wstate[cur],
             c->d_wres[cur], c->d_wlist[prv], wc, wc + WC_STRIDE, WK, n_tix, (int)rnd);
    }
    if (!c->tune.walk_rounds_fixed && c->wstat_n < 8) {         // the reads listed per round, kept for adapt_walk_rounds
      launch(c, k_wstat, dim3(1), dim3(32), 0, c->d_wctr, c->d_wstat + (size_t)c->wstat_n * 32, RM);
      c->wstat_pass[c->wstat_n] = pass; c->wstat_rm[c->wstat_n] = RM; c->wstat_n++;
    }
    if (c->tune.walk_debug) {                               // measurement aid: reads listed and tasks left per round, reads left to k_chain
      std::vector<unsigned long long> h((size_t)(RMX + 2) * WC_STRIDE);
      HIPCHK(c, hipMemcpyAsync(h.data(), c->d_wctr, h.size() * 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      { const unsigned long long* q = &h[(size_t)(RMX + 1) * WC_STRIDE];
        fprintf(stderr, "libsmr_hip: walk rounds (pass %d): slow %llu (positions <= 64 / 128 / 256 / 512 / more / > 64 hits: %llu %llu %llu %llu %llu %llu);", pass, q[0], q[8], q[9], q[10], q[11], q[12], q[13]); }
      for (uint32_t rnd = 0; rnd < RM; rnd++) fprintf(stderr, " %llu/%llu+%llu+%llu", h[(size_t)rnd * WC_STRIDE + WC_NLIST], h[(size_t)rnd * WC_STRIDE + WC_NTASK], h[(size_t)rnd * WC_STRIDE + WC_NTASK2], h[(size_t)rnd * WC_STRIDE + WC_NTASK3]);
      fprintf(stderr, "\n");
      unsigned long long ps[WPS_N];                         // (since smr_prof_reset, all launches of the context)
      HIPCHK(c, hipMemcpyAsync(ps, c->d_wpstat, sizeof ps, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(c, hipStreamSynchronize(c->stream));
      fprintf(stderr, "libsmr_hip: prefix tasks so far (SMR_WALK_PREFIX=%u): scored %llu decided %llu redone %llu; look-ahead tasks of reads expected to align under best N %llu, their cells %llu\n",
              c->tune.walk_prefix, ps[WPS_SCORED], ps[WPS_DECIDED], ps[WPS_REDONE], ps[WPS_AHEAD], ps[WPS_AHEAD_CELLS]);
    }
  }
  ev_mark(c, KP_CHAIN);
  // k_chain<EXT = false> over the marked reads; with the global tables on, k_chain<EXT = true> over the reads whose candidate set outgrew the LDS
  // table of the first launch: same walk, set in the block's global table
  for (int ext = 0; ext <= (c->chain_ext ? 1 : 0); ext++) {
    if (ext) HIPCHK(c, hipMemsetAsync(&B.d_ctr[C_WORK_NEXT], 0, 8, c->stream));
    if (c->cinfo_on) launch(c, k_cand_route, per_read, dim3(256), 0, B.n, B.d_marks, nullptr, nullptr, nullptr, 1 + ext, c->d_croute);
    launch(c, chain_kernel(ext, plan.lng, plan.striped), dim3(blocks), dim3(64), lds, dreads(c), dindex(di), P, pass, is_last_strand, B.d_work, B.d_work_aln, B.d_rw, c->d_pool, B.d_ctr,
           c->d_tuples, c->d_keys, c->d_pairs, c->d_lis, c->d_hits, c->keys_cap, c->pairs_cap, c->hits_cap, ml, rf, c->chain_scap, c->chain_ext ? c->d_stab.get() : nullptr,
           c->chain_ext ? c->d_tuples2.get() : nullptr, rq, gb, grd, B.d_marks, mrec, c->d_mpool, split ? c->d_wslow.get() : nullptr, n_slow);
  }
  ev_stop(c);
  HIPCHK(c, hipGetLastError());
  return SMR_OK;
}

// The begin cells of the alignments that are still stored (k_chain records the accepted ones "begin pending"): four reverse passes per wave, or --
// sixteen per wave through k_sw16 -- the end cells of the alignments stored end-pending (stage 0), then the begin cells of all (stage 1).
int launch_begins(smr_ctx* c, const DevIndex& di, const DParams& P, const AlignPlan& plan) {
  Batch& B = *c->b;
  int rc;
  const uint64_t ntot = (uint64_t)B.n * B.slots;
  if ((rc = c->d_tasks.reserve(c, 2 * ntot))) return rc;
  const int x4 = plan.x4 ? 1 : 0;
  const size_t lds_b = x4 ? (size_t)4 * (plan.ml + plan.rf) : (plan.lng ? 0 : (size_t)plan.ml + plan.rf);
  const uint32_t bg_blocks = (uint32_t)c->n_cu * 8u;
  if ((rc = ensure_bound(c, std::max(bg_blocks, c->chain_blocks), plan.rf))) return rc;
  if ((rc = raise_lds_limit(c, c->begins_lds_attr, lds_b, 64 * 1024, begins_kernel(0, 0), begins_kernel(1, 0), begins_kernel(0, 1), begins_kernel(1, 1)))) return rc;
  HIPCHK(c, hipMemsetAsync(&B.d_ctr[C_BEGIN_N], 0, 16, c->stream));       // C_BEGIN_N, C_BEGIN_NEXT
  ev_mark(c, KP_BEGINS);
  launch(c, k_begins_collect, dim3((uint32_t)((ntot + 1023) / 1024)), dim3(1024), 0, B.n, B.slots, B.d_work, B.d_rw, B.d_work_aln, c->d_tasks, B.d_ctr);
  const size_t task_cap = (size_t)c->walk_cap * c->walk_kcap;
  if (plan.begins_sw16 && c->d_wtask[0] && c->d_wctr && ntot <= task_cap) {
    for (int stage = 0; stage < 2; stage++) {
      HIPCHK(c, hipMemsetAsync(c->d_wctr, 0, (size_t)WC_STRIDE * 8, c->stream));
      launch(c, k_begins_prep, dim3((uint32_t)c->n_cu * 2u), dim3(1024), 0, dindex(di), B.slots, c->d_tasks, &B.d_ctr[C_BEGIN_N], B.d_work_aln, stage, c->d_wtask[0], c->d_wtidx, c->d_wctr);
      launch_sw16(c, plan.rows, 4, 0, dreads(c), dindex(di), P, c->d_wtask[0], c->d_wtidx, c->d_wtidx + task_cap, c->d_wtidx + 2 * task_cap, c->d_wctr, c->d_wres[0]);
      launch(c, k_begins_apply, dim3((uint32_t)c->n_cu * 4u), dim3(256), 0, c->d_tasks, &B.d_ctr[C_BEGIN_N], B.d_work_aln, stage, c->d_wtask[0], c->d_wres[0], B.d_ctr);
    }
  } else
    launch(c, begins_kernel(plan.lng, plan.striped), dim3(bg_blocks), dim3(64), lds_b, dreads(c), dindex(di), P, c->d_tasks, B.d_work_aln, B.d_ctr, plan.ml, plan.rf, x4,
           plan.lng ? c->d_bound.get() : nullptr, plan.lng ? c->d_rdq.get() : nullptr);
  ev_stop(c);
  return SMR_OK;
}

// fold the sharded work counters into their base slots (and clear the shards, so the vector can be written back);
// C_POOL_CURSOR becomes the largest shard cursor
void fold_shards(std::vector<unsigned long long>& h) {
  for (int s = 0; s < C_NSHARD; s++)
    for (int k = 0; k < C_SHARD_W; k++) {
      if (k < C_SHARD_X) h[C_WINDOWS + k] += h[C_SHARDS + C_SHARD_W * s + k];
      else if (k < C_SHARD_X + C_SHARD_NX) h[C_TUP_F + k - C_SHARD_X] += h[C_SHARDS + C_SHARD_W * s + k];
      else if (k >= C_SHARD_NB && k < C_SHARD_NB + 3) h[C_NB_PROBED + k - C_SHARD_NB] += h[C_SHARDS + C_SHARD_W * s + k];
      h[C_SHARDS + C_SHARD_W * s + k] = 0;
    }
  unsigned long long mx = 0;
  for (int s = 0; s < C_NSHARD; s++) mx = std::max(mx, h[C_PCUR + s * C_PCUR_STRIDE]);
  h[C_POOL_CURSOR] = mx;
}

int read_ctr(smr_ctx* c, std::vector<unsigned long long>& h) {
  h.resize(C_TOTAL);
  HIPCHK(c, hipMemcpyAsync(h.data(), c->b->d_ctr, C_TOTAL * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  fold_shards(h);
  return SMR_OK;
}

