// smr_engine_otu.hpp -- host side of smr_otu_part, smr_otu_sort_batch (kernels in smr_otu.hpp) and smr_fastx_denovo (k_fxs_dn_measure of
// smr_fxsplit.hpp); included by smr_engine.hip.  smr_otu_part: the members of otu_map.txt of one (index, part) over the selected batch,
// classified, compacted, sorted by reference and written on the device -- what smr_results_fetch + smr_reads_record_text + smr_result_record
// + smr_report_add do on the host one read at a time.  The host's share: two small copies back (the error counts, the two totals), then the
// bytes and the table of groups.

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
  if (!c || !need || !any_yid_ycov) return SMR_ERR_ARG;
  need[0] = need[1] = 0; *any_yid_ycov = 0;
  if (!ix || slot < 0 || slot >= 64) { set_err(c, "smr_otu_part: null index, or a slot outside 0..63"); return SMR_ERR_ARG; }
  if (!idcov_threshold_ok(min_id) || !idcov_threshold_ok(min_cov)) { set_err(c, "smr_otu_part: min_id and min_cov must be within [0, 1]"); return SMR_ERR_ARG; }
  if (!c->idx[slot].used || !c->b->d_saved) { set_err(c, "smr_otu_part: index slot empty or no reads uploaded"); return SMR_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  int rc = check_params(c, p, false); if (rc) return rc;
  DevIndex& di = c->idx[slot];
  if (di.n_refs != ix->n_refs() || di.ref_bytes != ix->ref_seq.size() || di.lnwin != ix->lnwin) { set_err(c, "smr_otu_part: `ix` is not the index part that is resident in the slot"); return SMR_ERR_ARG; }
  Batch& B = *c->b;
  if (!B.fx_kept) { set_err(c, "smr_otu_part: the batch does not hold its text (upload it with smr_reads_upload_fastx* and SMR_FASTX_KEEP)"); return SMR_ERR_STATE; }
  OtuScratch& S = c->otu;
  for (double& m : S.ms) m = 0.0;
  if (B.n == 0 || !B.d_idcov || B.d_idcov.cap() < (size_t)B.n * 4) return SMR_OK;      // (no pass: no counter is above 0)
  const uint64_t ntot = (uint64_t)B.n * B.slots;
  if (ntot >= 0xFFFFFC00ull) { set_err(c, "smr_otu_part: reads x alignment slots of the batch must stay below 2^32"); return SMR_ERR_CAPACITY; }
  for (auto& e : S.ev) if (!e) HIPCHK(c, hipEventCreate(&e));
  const uint32_t n = B.n, np = (n + OTU_BLOCK - 1u) / OTU_BLOCK;
  if ((rc = S.pass.reserve(c, ntot)) || (rc = S.meta.reserve(c, n)) || (rc = S.excl.reserve(c, n)) || (rc = S.part.reserve(c, (size_t)np + 1)) ||
      (rc = S.err.reserve(c, OTU_E_COUNT))) return rc;
  const unsigned long long pool_words = B.d_cigar ? B.cigar_words : 0ull;
  RowsSrc src; src.text = B.fx_text; src.n_text = B.fx_n; src.fastq = B.fx_fastq; src.hoff = B.fx_hoff; src.soff = B.fx_soff;
  const DReads rd = dreads(c);
  float f = 0;
  // 1. classify
  uint32_t h_err[OTU_E_COUNT];
  HIPCHK(c, hipMemsetAsync(S.err, 0, sizeof h_err, c->stream));
  HIPCHK(c, hipEventRecord(S.ev[0], c->stream));
  launch(c, k_otu_classify, dim3((uint32_t)std::min<uint64_t>((ntot + 15u) / 16u, (uint64_t)c->n_cu * 32u)), dim3(256), 0, rd, dindex(di), B.slots, (const RState*)B.d_saved,
         (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar, pool_words, (const uint32_t*)B.d_idcov, p->index_num, p->part, min_id, min_cov, S.pass, S.err);
  HIPCHK(c, hipEventRecord(S.ev[1], c->stream));
  // 2. size, scan, compact
  launch(c, k_otu_size, dim3(np), dim3(OTU_BLOCK), 0, n, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_idcov, (const uint8_t*)S.pass,
         p->index_num, p->part, src, S.meta, S.excl, S.part, S.err);
  launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.part, np + 1u);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(S.ev[9], c->stream));
  unsigned long long n_pairs = 0;
  HIPCHK(c, hipMemcpyAsync(h_err, S.err, sizeof h_err, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&n_pairs, S.part + np, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (hipEventElapsedTime(&f, S.ev[0], S.ev[1]) == hipSuccess) S.ms[0] = f;
  if (hipEventElapsedTime(&f, S.ev[1], S.ev[9]) == hipSuccess) S.ms[1] = f;
  if (h_err[OTU_E_NOCIG]) {
    set_err(c, "smr_otu_part: " + std::to_string(h_err[OTU_E_NOCIG]) + " alignments of this (index, part) have no CIGAR yet (call smr_traceback first)");
    return SMR_ERR_STATE;
  }
  if (h_err[OTU_E_BADREF]) { set_err(c, "smr_otu_part: " + std::to_string(h_err[OTU_E_BADREF]) + " alignments with ref_num out of range"); return SMR_ERR_ARG; }
  if (h_err[OTU_E_PAST]) { set_err(c, "smr_otu_part: " + std::to_string(h_err[OTU_E_PAST]) + " alignments whose CIGAR runs past its read or its reference"); return SMR_ERR_ARG; }
  *any_yid_ycov = h_err[OTU_E_ANY] != 0;
  if (n_pairs == 0) return SMR_OK;
  const uint32_t m = (uint32_t)n_pairs, mp = (m + OTU_BLOCK - 1u) / OTU_BLOCK;
  if ((rc = S.pairs.reserve(c, m)) || (rc = S.key[0].reserve(c, m)) || (rc = S.wexcl.reserve(c, m)) || (rc = S.gexcl.reserve(c, m)) ||
      (rc = S.wpart.reserve(c, (size_t)mp + 1)) || (rc = S.gpart.reserve(c, (size_t)mp + 1))) return rc;
  HIPCHK(c, hipEventRecord(S.ev[2], c->stream));
  launch(c, k_otu_pairs, dim3(np), dim3(OTU_BLOCK), 0, n, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_idcov, (const uint8_t*)S.pass,
         p->index_num, p->part, (const uint2*)S.meta, (const unsigned long long*)S.excl, (const unsigned long long*)S.part, S.key[0], S.pairs);
  HIPCHK(c, hipEventRecord(S.ev[3], c->stream));
  // 3. sort
  int where;
  if ((rc = otu_sort(c, m, otu_key_bits(di.n_refs), &where))) return rc;
  if (where < 0) {                                     // one reference: the order stands
    if ((rc = S.val[0].reserve(c, m))) return rc;
    launch(c, k_otu_iota, dim3((m + 255u) / 256u), dim3(256), 0, m, S.val[0]);
    where = 0;
  }
  HIPCHK(c, hipEventRecord(S.ev[4], c->stream));
  // 4. sizes of the text and of the table
  const uint32_t* keys = S.key[where]; const uint32_t* perm = S.val[where];
  launch(c, k_otu_wsize, dim3(mp), dim3(OTU_BLOCK), 0, m, keys, perm, (const uint4*)S.pairs, S.wexcl, S.wpart, S.gexcl, S.gpart);
  launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.wpart, mp + 1u);
  launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.gpart, mp + 1u);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(S.ev[5], c->stream));
  unsigned long long tot[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(&tot[0], S.wpart + mp, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&tot[1], S.gpart + mp, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (hipEventElapsedTime(&f, S.ev[2], S.ev[3]) == hipSuccess) S.ms[1] += f;
  if (hipEventElapsedTime(&f, S.ev[4], S.ev[5]) == hipSuccess) S.ms[1] += f;
  if (hipEventElapsedTime(&f, S.ev[3], S.ev[4]) == hipSuccess) S.ms[2] = f;
  need[0] = tot[0]; need[1] = tot[1];
  if (!bytes || !groups) return SMR_OK;
  if (cap < tot[0] || groups_cap < tot[1]) {
    set_err(c, "smr_otu_part: the map takes " + std::to_string(tot[0]) + " bytes and " + std::to_string(tot[1]) + " groups, the buffers have " + std::to_string(cap) + " and " +
                   std::to_string(groups_cap));
    return SMR_ERR_CAPACITY;
  }
  const uint32_t n_groups = (uint32_t)tot[1];
  if (S.out.cap() < tot[0] + 8u && (rc = S.out.alloc(c, (size_t)((tot[0] + (tot[0] >> 3) + 4095u) & ~4095ull)))) return rc;
  if ((rc = S.groups.reserve(c, n_groups)) || (rc = S.gstart.reserve(c, n_groups))) return rc;
  const uint32_t chunks = (m + 63u) / 64u, blocks = std::max(1u, std::min<uint32_t>((chunks + 3u) / 4u, (uint32_t)c->n_cu * 8u));
  HIPCHK(c, hipEventRecord(S.ev[6], c->stream));
  if (tot[0]) launch(c, k_otu_write, dim3(blocks), dim3(256), 0, m, keys, perm, (const uint4*)S.pairs, (const uint8_t*)B.fx_text, (const unsigned long long*)S.wexcl,
                     (const unsigned long long*)S.wpart, S.out);
  launch(c, k_otu_groups, dim3(mp), dim3(OTU_BLOCK), 0, m, keys, (const unsigned long long*)S.wexcl, (const unsigned long long*)S.wpart, (const unsigned long long*)S.gexcl,
         (const unsigned long long*)S.gpart, S.groups, S.gstart);
  launch(c, k_otu_gcount, dim3((n_groups + 255u) / 256u), dim3(256), 0, n_groups, m, (const uint32_t*)S.gstart, S.groups);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(S.ev[7], c->stream));
  if (tot[0]) HIPCHK(c, hipMemcpyAsync(bytes, S.out, (size_t)tot[0], hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(groups, S.groups, (size_t)n_groups * sizeof(OtuGroup), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(S.ev[8], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (hipEventElapsedTime(&f, S.ev[6], S.ev[7]) == hipSuccess) S.ms[3] = f;
  if (hipEventElapsedTime(&f, S.ev[7], S.ev[8]) == hipSuccess) S.ms[4] = f;
  return SMR_OK;
}

extern "C" int smr_otu_times(const smr_ctx* c, double ms[5]) {
  if (!c || !ms) return SMR_ERR_ARG;
  for (int k = 0; k < 5; k++) ms[k] = c->otu.ms[k];
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

// ---- aligned_denovo.* ------------------------------------------------------------------------------------------------------------------
namespace {
// smr_fastx_denovo (zip = false) and smr_fastx_denovo_gz (zip = true): as fxs_split_impl
int fxs_denovo_impl(smr_ctx* c, const char* who, bool zip, int mates, const smr_fxsplit_opts* o, const uint8_t* dn, uint8_t* bytes, uint64_t cap, uint64_t off[5],
                    uint64_t gz_off[5], uint64_t* need) {
  if (!c || !o || !off || (zip && (!gz_off || !need))) return SMR_ERR_ARG;
  const std::string W(who);
  for (int k = 0; k < 5; k++) off[k] = 0;
  if (zip) for (int k = 0; k < 5; k++) gz_off[k] = 0;
  if (need) *need = 0;
  if (o->layout < 0 || o->layout > 2) { set_err(c, W + ": layout must be 0 (single reads), 1 (mates interleaved) or 2 (mates in batch `mates`)"); return SMR_ERR_ARG; }
  Batch& A = *c->b;
  const Batch* M = nullptr;
  if (o->layout == 2) {
    if (mates < 0 || mates >= SMR_MAX_BATCHES || &c->bt[mates] == &A) { set_err(c, W + ": layout 2 takes the mates from another batch than the selected one"); return SMR_ERR_ARG; }
    M = &c->bt[mates];
  }
  if (o->layout != 0 && ((o->paired_in && o->paired_out) || (o->sout && (o->paired_in || o->paired_out)))) {      // what smr_report_open refuses
    set_err(c, W + ": invalid combination of paired_in / paired_out / sout"); return SMR_ERR_ARG;
  }
  if (!A.fx_kept || (M && !M->fx_kept)) {
    set_err(c, W + ": the batch does not hold its text (upload it with smr_reads_upload_fastx* and SMR_FASTX_KEEP)"); return SMR_ERR_STATE;
  }
  if (o->layout == 1 && (A.n & 1u)) { set_err(c, W + ": layout 1 with an odd number of reads (" + std::to_string(A.n) + ")"); return SMR_ERR_ARG; }
  if (M && M->n != A.n) { set_err(c, W + ": " + std::to_string(A.n) + " reads, " + std::to_string(M->n) + " mates"); return SMR_ERR_ARG; }
  if (M && M->fx_fastq != A.fx_fastq) { set_err(c, W + ": FASTA reads with FASTQ mates (or the other way round)"); return SMR_ERR_ARG; }
  const uint64_t n64 = (uint64_t)A.n * (M ? 2u : 1u);
  if (n64 >= 0xFFFFFFFFull) { set_err(c, W + ": 2^32 - 1 records or more"); return SMR_ERR_CAPACITY; }
  if (n64 == 0) return SMR_OK;
  HIPCHK(c, hipSetDevice(c->device));
  FxSplitScratch& S = c->fxs;
  const uint32_t n = (uint32_t)n64, np = (n + FXS_BLOCK - 1u) / FXS_BLOCK;
  int rc;
  if ((rc = S.rec.reserve(c, n)) || (rc = S.woff.reserve(c, n)) || (rc = S.part.reserve(c, (size_t)np * 8u)) || (rc = S.tot.reserve(c, 9))) return rc;
  if (dn) {
    if ((rc = S.hit.reserve(c, n))) return rc;
    HIPCHK(c, hipMemcpyAsync(S.hit, dn, n, hipMemcpyHostToDevice, c->stream));
  }
  FxsOpts D;
  D.layout = (uint32_t)o->layout; D.fastq = A.fx_fastq; D.paired_in = o->paired_in != 0; D.paired_out = o->paired_out != 0; D.out2 = o->out2 != 0; D.sout = o->sout != 0;
  D.want_aligned = 1; D.want_other = 0;
  const FxsSrc a = fxs_src(A), b = fxs_src(M ? *M : A);
  // the counters of a batch on which the pass never ran hold nothing: no de novo read
  auto counters = [](const Batch& X) { return X.d_idcov && X.d_idcov.cap() >= (size_t)X.n * 4 ? (const uint32_t*)X.d_idcov : (const uint32_t*)nullptr; };
  launch(c, k_fxs_dn_measure, dim3(np), dim3(FXS_BLOCK), 0, n, D, a, b, counters(A), counters(M ? *M : A), dn ? (const uint8_t*)S.hit : (const uint8_t*)nullptr, S.rec, S.woff, S.part);
  launch(c, k_fxs_scan, dim3(1), dim3(FXS_BLOCK), 0, S.part, np, S.tot);
  HIPCHK(c, hipGetLastError());
  unsigned long long h_tot[9];
  HIPCHK(c, hipMemcpyAsync(h_tot, S.tot, sizeof h_tot, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 5; k++) off[k] = h_tot[k];
  const uint64_t total = h_tot[4];                     // (streams 4..7 stay empty: tot[4..8] all hold the end of stream 3)
  if (need) *need = total;
  if (zip) {
    *need = 0;
    if (total == 0) return SMR_OK;
    if (S.out.cap() < total + 4u && (rc = S.out.alloc(c, (size_t)((total + (total >> 3) + 4095u) & ~4095ull)))) return rc;
    const uint32_t quads = (n + 3u) / 4u, blocks = std::max(1u, std::min<uint32_t>((quads + 3u) / 4u, (uint32_t)c->n_cu * 16u));
    launch(c, k_fxs_copy, dim3(blocks), dim3(256), 0, n, D, a, b, (const uint4*)S.rec, (const unsigned long long*)S.woff, (const unsigned long long*)S.part,
           (const unsigned long long*)S.tot, S.out);
    HIPCHK(c, hipGetLastError());
    return gz_run(c, who, S.out, off, 4, bytes, cap, gz_off, need);
  }
  if (!bytes) return SMR_OK;
  if (cap < total) { set_err(c, W + ": the streams take " + std::to_string(total) + " bytes, the buffer has " + std::to_string(cap)); return SMR_ERR_CAPACITY; }
  if (total == 0) return SMR_OK;
  if (S.out.cap() < total + 4u && (rc = S.out.alloc(c, (size_t)((total + (total >> 3) + 4095u) & ~4095ull)))) return rc;
  const uint32_t quads = (n + 3u) / 4u, blocks = std::max(1u, std::min<uint32_t>((quads + 3u) / 4u, (uint32_t)c->n_cu * 16u));
  launch(c, k_fxs_copy, dim3(blocks), dim3(256), 0, n, D, a, b, (const uint4*)S.rec, (const unsigned long long*)S.woff, (const unsigned long long*)S.part,
         (const unsigned long long*)S.tot, S.out);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(bytes, S.out, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SMR_OK;
}
}  // namespace
extern "C" int smr_fastx_denovo(smr_ctx* c, int mates, const smr_fxsplit_opts* o, const uint8_t* dn, uint8_t* bytes, uint64_t cap, uint64_t off[5], uint64_t* need) {
  return fxs_denovo_impl(c, "smr_fastx_denovo", false, mates, o, dn, bytes, cap, off, nullptr, need);
}
extern "C" int smr_fastx_denovo_gz(smr_ctx* c, int mates, const smr_fxsplit_opts* o, const uint8_t* dn, uint8_t* gz, uint64_t cap, uint64_t gz_off[5], uint64_t plain_off[5],
                                   uint64_t* need) {
  return fxs_denovo_impl(c, "smr_fastx_denovo_gz", true, mates, o, dn, gz, cap, plain_off, gz_off, need);
}
