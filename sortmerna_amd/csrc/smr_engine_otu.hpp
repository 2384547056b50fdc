// smr_engine_otu.hpp -- host side of smr_otu_part and smr_otu_sort_batch (kernels in smr_otu.hpp); included by smr_engine.hip behind
// smr_engine_rows.hpp, whose PartCall preamble and refusals it uses.  smr_otu_part: the members of otu_map.txt of one (index, part) over the
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
  if (B.n == 0 || !B.d_idcov || B.d_idcov.cap() < (size_t)B.n * 4) return SMR_OK;      // (no pass: no counter is above 0)
  if ((rc = part_call_views(c, who, pc))) return rc;
  const uint32_t n = pc.n, np = (n + OTU_BLOCK - 1u) / OTU_BLOCK;
  if ((rc = S.pass.reserve(c, pc.ntot)) || (rc = S.meta.reserve(c, n)) || (rc = S.excl.reserve(c, n)) || (rc = S.part.reserve(c, (size_t)np + 1)) ||
      (rc = S.err.reserve(c, OTU_E_COUNT))) return rc;
  // 1. classify
  uint32_t h_err[OTU_E_COUNT];
  HIPCHK(c, hipMemsetAsync(S.err, 0, sizeof h_err, c->stream));
  if ((rc = T.mark(c, 0, c->stream))) return rc;
  launch(c, k_otu_classify, dim3((uint32_t)std::min<uint64_t>((pc.ntot + 15u) / 16u, (uint64_t)c->n_cu * 32u)), dim3(256), 0, pc.rd, pc.dx, B.slots, (const RState*)B.d_saved,
         (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar, pc.pool_words, (const uint32_t*)B.d_idcov, p->index_num, p->part, min_id, min_cov, S.pass, S.err);
  if ((rc = T.mark(c, 1, c->stream))) return rc;
  // 2. size, scan, compact
  launch(c, k_otu_size, dim3(np), dim3(OTU_BLOCK), 0, n, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_idcov, (const uint8_t*)S.pass,
         p->index_num, p->part, pc.src, S.meta, S.excl, S.part, S.err);
  launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.part, np + 1u);
  HIPCHK(c, hipGetLastError());
  if ((rc = T.mark(c, 9, c->stream))) return rc;
  unsigned long long n_pairs = 0;
  HIPCHK(c, hipMemcpyAsync(h_err, S.err, sizeof h_err, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&n_pairs, S.part + np, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  T.set(0, 0, 1);
  T.set(1, 1, 9);
  if ((rc = part_refuse_state(c, who, h_err[OTU_E_NOCIG], h_err[OTU_E_BADREF], h_err[OTU_E_PAST]))) return rc;
  *any_yid_ycov = h_err[OTU_E_ANY] != 0;
  if (n_pairs == 0) return SMR_OK;
  const uint32_t m = (uint32_t)n_pairs, mp = (m + OTU_BLOCK - 1u) / OTU_BLOCK;
  if ((rc = S.pairs.reserve(c, m)) || (rc = S.key[0].reserve(c, m)) || (rc = S.wexcl.reserve(c, m)) || (rc = S.gexcl.reserve(c, m)) ||
      (rc = S.wpart.reserve(c, (size_t)mp + 1)) || (rc = S.gpart.reserve(c, (size_t)mp + 1))) return rc;
  if ((rc = T.mark(c, 2, c->stream))) return rc;
  launch(c, k_otu_pairs, dim3(np), dim3(OTU_BLOCK), 0, n, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_idcov, (const uint8_t*)S.pass,
         p->index_num, p->part, (const uint2*)S.meta, (const unsigned long long*)S.excl, (const unsigned long long*)S.part, S.key[0], S.pairs);
  if ((rc = T.mark(c, 3, c->stream))) return rc;
  // 3. sort
  int where;
  if ((rc = otu_sort(c, m, otu_key_bits(pc.di.n_refs), &where))) return rc;
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
    set_err(c, "smr_otu_part: the map takes " + std::to_string(tot[0]) + " bytes and " + std::to_string(tot[1]) + " groups, the buffers have " + std::to_string(cap) + " and " +
                   std::to_string(groups_cap));
    return SMR_ERR_CAPACITY;
  }
  const uint32_t n_groups = (uint32_t)tot[1];
  if ((rc = S.out.reserve_headroom(c, (size_t)tot[0], 8))) return rc;
  if ((rc = S.groups.reserve(c, n_groups)) || (rc = S.gstart.reserve(c, n_groups))) return rc;
  const uint32_t chunks = (m + 63u) / 64u, blocks = std::max(1u, std::min<uint32_t>((chunks + 3u) / 4u, (uint32_t)c->n_cu * 8u));
  if ((rc = T.mark(c, 6, c->stream))) return rc;
  if (tot[0]) launch(c, k_otu_write, dim3(blocks), dim3(256), 0, m, keys, perm, (const uint4*)S.pairs, (const uint8_t*)B.fx_text, (const unsigned long long*)S.wexcl,
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

extern "C" int smr_otu_times(const smr_ctx* c, double ms[5]) {
  if (!c || !ms) return SMR_ERR_ARG;
  c->otu.clk.copy_to(ms);
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
