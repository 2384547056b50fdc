// smr_engine_otu.hpp -- host side of smr_otu_part, smr_otu_part_mates and smr_otu_sort_batch (kernels in smr_otu.hpp, smr_otu_mates.hpp); included by
// smr_engine.hip behind smr_engine_rows.hpp and smr_engine_mates.hpp, whose PartCall preamble and refusals it uses.  smr_otu_part: the members of otu_map.txt of one (index, part) over the
// selected batch, classified, compacted, sorted by reference and written on the device -- what smr_results_fetch + smr_reads_record_text +
// smr_result_record + smr_report_add do on the host one read at a time.  The host's share: two small copies back (the error counts, the two
// totals), then the bytes and the table of groups.  (smr_fastx_denovo lives with its siblings in smr_engine_fxsplit.hpp.)

static_assert(sizeof(smr_otu_group) == sizeof(OtuGroup) && offsetof(smr_otu_group, off) == offsetof(OtuGroup, off), "smr_otu_group is OtuGroup");

namespace {
// the stable sort of keys[0 .. n) (in S.key[0]) by their low key_bits bits: -> which of S.key[] / S.val[] holds the result; -1: no pass ran,
// the order is the input's and S.val holds nothing
int otu_sort(smr_ctx* c, uint32_t n, uint32_t key_bits, int* where) {
  OtuScratch& S = c->otu;
  *where = -1;
  const uint32_t passes = (key_bits + 7u) / 8u;
  if (n == 0 || passes == 0) return SMR_OK;
  const uint32_t n_units = (n + OTU_UNIT - 1u) / OTU_UNIT, blocks = (n_units + 3u) / 4u;
  int rc;
  if ((rc = S.key[1].reserve(c, n)) || (rc = S.val[0].reserve(c, n)) || (rc = S.val[1].reserve(c, n)) || (rc = S.hist.reserve(c, (size_t)n_units * 256u))) return rc;
  int cur = 0;
  for (uint32_t ps = 0; ps < passes; ps++, cur ^= 1) {
    launch(c, k_otu_hist, dim3(blocks), dim3(256), 0, n, (const uint32_t*)S.key[cur], 8u * ps, n_units, S.hist);
    launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.hist, n_units * 256u);
    launch(c, k_otu_move, dim3(blocks), dim3(256), 0, n, (const uint32_t*)S.key[cur], ps ? (const uint32_t*)S.val[cur] : (const uint32_t*)nullptr, 8u * ps, n_units,
           (const unsigned long long*)S.hist, S.key[cur ^ 1], S.val[cur ^ 1]);
  }
  HIPCHK(c, hipGetLastError());
  *where = cur;
  return SMR_OK;
}
uint32_t otu_key_bits(uint32_t n_refs) {
  uint32_t b = 0;
  while (b < 32u && ((uint64_t)1 << b) < (uint64_t)n_refs) b++;      // keys are below n_refs
  return b;
}
}  // namespace

namespace {
// the per-read scratch of one batch: what k_otu_classify and k_otu_size leave
struct OtuRead { DevBuf<uint8_t>& pass; DevBuf<uint2>& meta; DevBuf<unsigned long long>& excl; DevBuf<unsigned long long>& part; };
bool otu_has_pass(const Batch& B) { return B.n != 0 && B.d_idcov && B.d_idcov.cap() >= (size_t)B.n * 4; }

// stages 1 and 2 over the batch of `pc` (views made): classify, size, scan -- events 0, 1 and 9 of T, its times 0 and 1 -- and the refusal of state
// the writers would read out of bounds for.  -> the members of the batch, and whether one of its reads has c_yid_ycov > 0
int otu_members(smr_ctx* c, const char* who, StageClock<10, 5>& T, const PartCall& pc, const OtuRead& R, const smr_params* p, double min_id, double min_cov,
                unsigned long long* n_pairs, int* any) {
  const Batch& B = pc.B;
  OtuScratch& S = c->otu;
  const uint32_t n = pc.n, np = (n + OTU_BLOCK - 1u) / OTU_BLOCK;
  int rc;
  if ((rc = R.pass.reserve(c, pc.ntot)) || (rc = R.meta.reserve(c, n)) || (rc = R.excl.reserve(c, n)) || (rc = R.part.reserve(c, (size_t)np + 1)) ||
      (rc = S.err.reserve(c, OTU_E_COUNT))) return rc;
  // 1. classify
  uint32_t h_err[OTU_E_COUNT];
  HIPCHK(c, hipMemsetAsync(S.err, 0, sizeof h_err, c->stream));
  if ((rc = T.mark(c, 0, c->stream))) return rc;
  launch(c, k_otu_classify, dim3((uint32_t)std::min<uint64_t>((pc.ntot + 15u) / 16u, (uint64_t)c->n_cu * 32u)), dim3(256), 0, pc.rd, pc.dx, B.slots, (const RState*)B.d_saved,
         (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar, pc.pool_words, (const uint32_t*)B.d_idcov, p->index_num, p->part, min_id, min_cov, R.pass, S.err);
  if ((rc = T.mark(c, 1, c->stream))) return rc;
  // 2. size, scan
  launch(c, k_otu_size, dim3(np), dim3(OTU_BLOCK), 0, n, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_idcov, (const uint8_t*)R.pass,
         p->index_num, p->part, pc.src, R.meta, R.excl, R.part, S.err);
  launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, R.part, np + 1u);
  HIPCHK(c, hipGetLastError());
  if ((rc = T.mark(c, 9, c->stream))) return rc;
  *n_pairs = 0;
  HIPCHK(c, hipMemcpyAsync(h_err, S.err, sizeof h_err, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(n_pairs, R.part + np, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  T.set(0, 0, 1);
  T.set(1, 1, 9);
  if ((rc = part_refuse_state(c, who, h_err[OTU_E_NOCIG], h_err[OTU_E_BADREF], h_err[OTU_E_PAST]))) return rc;
  *any = h_err[OTU_E_ANY] != 0;
  return SMR_OK;
}

// stages 3 and 4 over the m members in S.pairs / S.key[0] (events 3 .. 8 of S.clk; event 3 is marked): sort, sizes, text and table, D2H.
// text_m: the text of the members with OTU_MATE_BIT (null: there are none, k_otu_write)
int otu_finish(smr_ctx* c, const char* who, uint32_t m, uint32_t n_refs, const uint8_t* text, const uint8_t* text_m, uint8_t* bytes, uint64_t cap, smr_otu_group* groups,
               uint64_t groups_cap, uint64_t need[2]) {
  OtuScratch& S = c->otu;
  StageClock<10, 5>& T = S.clk;
  const uint32_t mp = (m + OTU_BLOCK - 1u) / OTU_BLOCK;
  // 3. sort
  int rc, where;
  if ((rc = otu_sort(c, m, otu_key_bits(n_refs), &where))) return rc;
  if (where < 0) {                                     // one reference: the order stands
    if ((rc = S.val[0].reserve(c, m))) return rc;
    launch(c, k_otu_iota, dim3((m + 255u) / 256u), dim3(256), 0, m, S.val[0]);
    where = 0;
  }
  if ((rc = T.mark(c, 4, c->stream))) return rc;
  // 4. sizes of the text and of the table
  const uint32_t* keys = S.key[where]; const uint32_t* perm = S.val[where];
  launch(c, k_otu_wsize, dim3(mp), dim3(OTU_BLOCK), 0, m, keys, perm, (const uint4*)S.pairs, S.wexcl, S.wpart, S.gexcl, S.gpart);
  launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.wpart, mp + 1u);
  launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.gpart, mp + 1u);
  HIPCHK(c, hipGetLastError());
  if ((rc = T.mark(c, 5, c->stream))) return rc;
  unsigned long long tot[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(&tot[0], S.wpart + mp, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&tot[1], S.gpart + mp, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  T.add(1, 2, 3);
  T.add(1, 4, 5);
  T.set(2, 3, 4);
  need[0] = tot[0]; need[1] = tot[1];
  if (!bytes || !groups) return SMR_OK;
  if (cap < tot[0] || groups_cap < tot[1]) {
    set_err(c, std::string(who) + ": the map takes " + std::to_string(tot[0]) + " bytes and " + std::to_string(tot[1]) + " groups, the buffers have " + std::to_string(cap) +
                   " and " + std::to_string(groups_cap));
    return SMR_ERR_CAPACITY;
  }
  const uint32_t n_groups = (uint32_t)tot[1];
  if ((rc = S.out.reserve_headroom(c, (size_t)tot[0], 8))) return rc;
  if ((rc = S.groups.reserve(c, n_groups)) || (rc = S.gstart.reserve(c, n_groups))) return rc;
  const uint32_t chunks = (m + 63u) / 64u, blocks = std::max(1u, std::min<uint32_t>((chunks + 3u) / 4u, (uint32_t)c->n_cu * 8u));
  if ((rc = T.mark(c, 6, c->stream))) return rc;
  if (tot[0] && !text_m) launch(c, k_otu_write, dim3(blocks), dim3(256), 0, m, keys, perm, (const uint4*)S.pairs, text, (const unsigned long long*)S.wexcl,
                                (const unsigned long long*)S.wpart, S.out);
  if (tot[0] && text_m) launch(c, k_otu_mates_write, dim3(blocks), dim3(256), 0, m, keys, perm, (const uint4*)S.pairs, text, text_m, (const unsigned long long*)S.wexcl,
                               (const unsigned long long*)S.wpart, S.out);
  launch(c, k_otu_groups, dim3(mp), dim3(OTU_BLOCK), 0, m, keys, (const unsigned long long*)S.wexcl, (const unsigned long long*)S.wpart, (const unsigned long long*)S.gexcl,
         (const unsigned long long*)S.gpart, S.groups, S.gstart);
  launch(c, k_otu_gcount, dim3((n_groups + 255u) / 256u), dim3(256), 0, n_groups, m, (const uint32_t*)S.gstart, S.groups);
  HIPCHK(c, hipGetLastError());
  if ((rc = T.mark(c, 7, c->stream))) return rc;
  if (tot[0]) HIPCHK(c, hipMemcpyAsync(bytes, S.out, (size_t)tot[0], hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(groups, S.groups, (size_t)n_groups * sizeof(OtuGroup), hipMemcpyDeviceToHost, c->stream));
  if ((rc = T.mark(c, 8, c->stream))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  T.set(3, 6, 7);
  T.set(4, 7, 8);
  return SMR_OK;
}
}  // namespace

extern "C" int smr_otu_part(smr_ctx* c, int slot, const smr_params* p, const smr_index* ix, double min_id, double min_cov,
                            uint8_t* bytes, uint64_t cap, smr_otu_group* groups, uint64_t groups_cap, uint64_t need[2], int* any_yid_ycov) {
  static const char* const who = "smr_otu_part";
  if (!c || !need || !any_yid_ycov) return SMR_ERR_ARG;
  need[0] = need[1] = 0; *any_yid_ycov = 0;
  if (!ix || slot < 0 || slot >= 64) { set_err(c, "smr_otu_part: null index, or a slot outside 0..63"); return SMR_ERR_ARG; }
  if (!idcov_threshold_ok(min_id) || !idcov_threshold_ok(min_cov)) { set_err(c, "smr_otu_part: min_id and min_cov must be within [0, 1]"); return SMR_ERR_ARG; }
  PartCall pc = {c->idx[slot], *c->b};
  int rc = part_call_open(c, who, p, ix, pc); if (rc) return rc;
  const Batch& B = pc.B;
  OtuScratch& S = c->otu;
  StageClock<10, 5>& T = S.clk;
  if ((rc = T.begin(c))) return rc;
  S.last_mates = false;
  if (!otu_has_pass(B)) return SMR_OK;                  // (no reads, or no pass: no counter is above 0)
  if ((rc = part_call_views(c, who, pc))) return rc;
  const uint32_t n = pc.n, np = (n + OTU_BLOCK - 1u) / OTU_BLOCK;
  unsigned long long n_pairs = 0;
  if ((rc = otu_members(c, who, T, pc, OtuRead{S.pass, S.meta, S.excl, S.part}, p, min_id, min_cov, &n_pairs, any_yid_ycov))) return rc;
  if (n_pairs == 0) return SMR_OK;
  const uint32_t m = (uint32_t)n_pairs, mp = (m + OTU_BLOCK - 1u) / OTU_BLOCK;
  if ((rc = S.pairs.reserve(c, m)) || (rc = S.key[0].reserve(c, m)) || (rc = S.wexcl.reserve(c, m)) || (rc = S.gexcl.reserve(c, m)) ||
      (rc = S.wpart.reserve(c, (size_t)mp + 1)) || (rc = S.gpart.reserve(c, (size_t)mp + 1))) return rc;
  if ((rc = T.mark(c, 2, c->stream))) return rc;
  launch(c, k_otu_pairs, dim3(np), dim3(OTU_BLOCK), 0, n, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_idcov, (const uint8_t*)S.pass,
         p->index_num, p->part, (const uint2*)S.meta, (const unsigned long long*)S.excl, (const unsigned long long*)S.part, S.key[0], S.pairs);
  if ((rc = T.mark(c, 3, c->stream))) return rc;
  return otu_finish(c, who, m, pc.di.n_refs, (const uint8_t*)B.fx_text, nullptr, bytes, cap, groups, groups_cap, need);
}

// smr_otu_part for mates read from two files (kernels in smr_otu_mates.hpp): read i of the selected batch is mate 1 of pair i, read i of batch
// `mates` its mate 2.  Classify and size run over either batch with a scratch set of its own (S.pass .. S.part, S.pass_m .. S.part_m),
// k_otu_mates_pairs merges the members in the order of smr_report_add_pair, and the plain call's sort and writer take them from there.  The
// refusals come in the precedence of smr_rows_part_mates (mates_arg, mates_open of smr_engine_mates.hpp).  No call here selects a batch.
extern "C" int smr_otu_part_mates(smr_ctx* c, int mates, int slot, const smr_params* p, const smr_index* ix, double min_id, double min_cov,
                                  uint8_t* bytes, uint64_t cap, smr_otu_group* groups, uint64_t groups_cap, uint64_t need[2], int* any_yid_ycov) {
  static const char* const who = "smr_otu_part_mates";
  const std::string W = std::string(who) + ": ";
  if (!c || !need || !any_yid_ycov) return SMR_ERR_ARG;
  need[0] = need[1] = 0; *any_yid_ycov = 0;
  if (!ix || !p || slot < 0 || slot >= 64) { set_err(c, W + "null parameters or index, or a slot outside 0..63"); return SMR_ERR_ARG; }
  int rc = mates_arg(c, W, mates); if (rc) return rc;
  if (!idcov_threshold_ok(min_id) || !idcov_threshold_ok(min_cov)) { set_err(c, W + "min_id and min_cov must be within [0, 1]"); return SMR_ERR_ARG; }
  Batch& A = *c->b;
  Batch& M = c->bt[mates];
  const std::string who_m = std::string(who) + " (batch " + std::to_string(mates) + ")";
  PartCall pa = {c->idx[slot], A}, pm = {c->idx[slot], M};
  if ((rc = part_call_open(c, who, p, ix, pa))) return rc;
  OtuScratch& S = c->otu;
  StageClock<10, 5>&T = S.clk, &TA = S.clk_ab[0], &TM = S.clk_ab[1];
  if ((rc = T.begin(c)) || (rc = TA.begin(c)) || (rc = TM.begin(c))) return rc;
  S.last_mates = true; S.compact_ms = 0.0;
  const bool has_a = otu_has_pass(A);
  unsigned long long na = 0, nb = 0;
  int any_a = 0, any_b = 0;
  if (has_a) {                                         // the plain call's stages, and with them its refusals, for the selected batch
    if ((rc = part_call_views(c, who, pa))) return rc;
    if ((rc = otu_members(c, who, TA, pa, OtuRead{S.pass, S.meta, S.excl, S.part}, p, min_id, min_cov, &na, &any_a))) return rc;
  }
  if ((rc = mates_open(c, W, mates, A, M))) return rc;
  if (A.n == 0) return SMR_OK;
  if (A.n >= OTU_MATE_BIT) { set_err(c, W + "the reads of a batch must stay below 2^31"); return SMR_ERR_CAPACITY; }
  const bool has_b = otu_has_pass(M);
  if (has_b) {
    if ((rc = part_call_views(c, who_m.c_str(), pm))) return rc;
    if ((rc = otu_members(c, who_m.c_str(), TM, pm, OtuRead{S.pass_m, S.meta_m, S.excl_m, S.part_m}, p, min_id, min_cov, &nb, &any_b))) return rc;
  }
  *any_yid_ycov = any_a | any_b;
  double ta[5], tm[5];
  TA.copy_to(ta); TM.copy_to(tm);
  T.acc(0, ta[0] + tm[0]);
  T.acc(1, ta[1] + tm[1]);
  if (na + nb == 0) return SMR_OK;
  if (na + nb > 0xFFFFFFFFull) { set_err(c, W + "the members of the two batches must stay below 2^32"); return SMR_ERR_CAPACITY; }
  const uint32_t n = A.n, np = (n + OTU_BLOCK - 1u) / OTU_BLOCK;
  const uint32_t m = (uint32_t)(na + nb), mp = (m + OTU_BLOCK - 1u) / OTU_BLOCK;
  // a batch on which the pass never ran has no members: zeros where k_otu_mates_pairs looks for its sums
  if (!has_a) {
    if ((rc = S.excl.reserve(c, n)) || (rc = S.part.reserve(c, (size_t)np + 1))) return rc;
    HIPCHK(c, hipMemsetAsync(S.excl, 0, (size_t)n * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(S.part, 0, ((size_t)np + 1) * 8, c->stream));
  }
  if (!has_b) {
    if ((rc = S.excl_m.reserve(c, n)) || (rc = S.part_m.reserve(c, (size_t)np + 1))) return rc;
    HIPCHK(c, hipMemsetAsync(S.excl_m, 0, (size_t)n * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(S.part_m, 0, ((size_t)np + 1) * 8, c->stream));
  }
  if ((rc = S.pairs.reserve(c, m)) || (rc = S.key[0].reserve(c, m)) || (rc = S.wexcl.reserve(c, m)) || (rc = S.gexcl.reserve(c, m)) ||
      (rc = S.wpart.reserve(c, (size_t)mp + 1)) || (rc = S.gpart.reserve(c, (size_t)mp + 1))) return rc;
  const OtuSide sa = {A.slots, (const RState*)A.d_saved, (const AlignRec*)A.d_saved_aln, (const uint8_t*)S.pass, (const uint2*)S.meta, (const unsigned long long*)S.excl,
                      (const unsigned long long*)S.part};
  const OtuSide sm = {M.slots, (const RState*)M.d_saved, (const AlignRec*)M.d_saved_aln, (const uint8_t*)S.pass_m, (const uint2*)S.meta_m, (const unsigned long long*)S.excl_m,
                      (const unsigned long long*)S.part_m};
  if ((rc = T.mark(c, 2, c->stream))) return rc;
  launch(c, k_otu_mates_pairs, dim3(np, 2), dim3(OTU_BLOCK), 0, n, sa, sm, p->index_num, p->part, S.key[0], S.pairs);
  if ((rc = T.mark(c, 3, c->stream))) return rc;
  rc = otu_finish(c, who, m, pa.di.n_refs, (const uint8_t*)A.fx_text, (const uint8_t*)M.fx_text, bytes, cap, groups, groups_cap, need);
  (void)T.elapsed(2, 3, S.compact_ms);                 // (otu_finish has synchronised the stream behind event 3, or failed in front of that)
  return rc;
}

extern "C" int smr_otu_times(const smr_ctx* c, double ms[5]) {
  if (!c || !ms) return SMR_ERR_ARG;
  c->otu.clk.copy_to(ms);
  return SMR_OK;
}

extern "C" int smr_otu_mates_times(const smr_ctx* c, double ms[5]) {
  if (!c || !ms) return SMR_ERR_ARG;
  for (int k = 0; k < 5; k++) ms[k] = 0.0;
  if (!c->otu.last_mates) return SMR_OK;
  double t[5];
  c->otu.clk_ab[0].copy_to(t); ms[0] = t[0]; ms[1] = t[1];
  c->otu.clk_ab[1].copy_to(t); ms[2] = t[0]; ms[3] = t[1];
  ms[4] = c->otu.compact_ms;
  return SMR_OK;
}

extern "C" int smr_otu_sort_batch(smr_ctx* c, uint32_t n, const uint32_t* keys, uint32_t key_bits, uint32_t* perm) {
  if (!c) return SMR_ERR_ARG;
  if (key_bits > 32u) { set_err(c, "smr_otu_sort_batch: key_bits above 32"); return SMR_ERR_ARG; }
  if (n == 0) return SMR_OK;
  if (!keys || !perm) return SMR_ERR_ARG;
  if (key_bits < 32u) for (uint32_t i = 0; i < n; i++) if (keys[i] >> key_bits) { set_err(c, "smr_otu_sort_batch: a key of more than key_bits bits"); return SMR_ERR_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  OtuScratch& S = c->otu;
  int rc, where;
  if ((rc = S.key[0].reserve(c, n))) return rc;
  HIPCHK(c, hipMemcpyAsync(S.key[0], keys, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  if ((rc = otu_sort(c, n, key_bits, &where))) return rc;
  if (where < 0) { HIPCHK(c, hipStreamSynchronize(c->stream)); for (uint32_t i = 0; i < n; i++) perm[i] = i; return SMR_OK; }
  HIPCHK(c, hipMemcpyAsync(perm, S.val[where], (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SMR_OK;
}
