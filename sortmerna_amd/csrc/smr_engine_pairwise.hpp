// smr_engine_pairwise.hpp -- host side of smr_pairwise_part (included by smr_engine.hip behind smr_engine_rows.hpp; kernels in smr_pairwise.hpp):
// the BLAST-like pairwise text (-blast 0) of one (index, part) over the selected batch, guarded, sized and written on the device -- what
// smr_results_fetch + smr_reads_record_text + smr_result_record + smr_report_add do on the host one read at a time.  The host's share is that of
// smr_rows_part, whose pieces are used as they are: the names of the part's references (rows_names), the e-value / bit-score texts per score
// (rows_table), the guards of k_rows_stat, the device buffers of RowsScratch; two small copies back (the error counts, the total) and the bytes.

extern "C" int smr_pairwise_part(smr_ctx* c, int slot, const smr_params* p, const smr_index* ix, double lambda, double K, uint64_t full_ref_corr,
                                 uint64_t full_read_corr, uint8_t* bytes, uint64_t cap, uint64_t* need) {
  static const char* const who = "smr_pairwise_part";
  if (!c || !need) return SMR_ERR_ARG;
  *need = 0;
  if (!ix || slot < 0 || slot >= 64) { set_err(c, "smr_pairwise_part: null index, or a slot outside 0..63"); return SMR_ERR_ARG; }
  if (!c->idx[slot].used || !c->b->d_saved) { set_err(c, "smr_pairwise_part: index slot empty or no reads uploaded"); return SMR_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  int rc = check_params(c, p, false); if (rc) return rc;
  DevIndex& di = c->idx[slot];
  if (di.n_refs != ix->n_refs() || di.ref_bytes != ix->ref_seq.size() || di.lnwin != ix->lnwin) { set_err(c, "smr_pairwise_part: `ix` is not the index part that is resident in the slot"); return SMR_ERR_ARG; }
  Batch& B = *c->b;
  if (!B.fx_kept) { set_err(c, "smr_pairwise_part: the batch does not hold its text (upload it with smr_reads_upload_fastx* and SMR_FASTX_KEEP)"); return SMR_ERR_STATE; }
  if (B.n == 0) return SMR_OK;
  const uint64_t ntot = (uint64_t)B.n * B.slots;
  if (ntot >= 0xFFFFFC00ull) { set_err(c, "smr_pairwise_part: reads x alignment slots of the batch must stay below 2^32"); return SMR_ERR_CAPACITY; }
  RowsOpts D;
  memset(&D, 0, sizeof D);
  D.want_blast = 1; D.index_num = p->index_num; D.part = p->part;       // (want_blast: k_rows_stat checks the scores against the table)
  smr_rows_opts db;
  memset(&db, 0, sizeof db);
  db.lambda = lambda; db.K = K; db.full_ref_corr = full_ref_corr; db.full_read_corr = full_read_corr;
  RowsScratch& S = c->rows;
  PairScratch& T = c->pair;
  for (auto& e : T.ev) if (!e) HIPCHK(c, hipEventCreate(&e));
  for (double& m : T.ms) m = 0.0;
  const uint32_t n = B.n, np = (n + ROWS_BLOCK - 1u) / ROWS_BLOCK;
  if ((rc = rows_names(c, di, ix, p->part, who))) return rc;
  D.n_tab = (uint32_t)std::min<uint64_t>(65536u, (uint64_t)p->match * B.max_len + 1u);
  if ((rc = rows_table(c, &db, D.n_tab, who))) return rc;
  if ((rc = S.stat.reserve(c, ntot)) || (rc = S.meta.reserve(c, n)) || (rc = S.excl_b.reserve(c, n)) || (rc = S.part_b.reserve(c, (size_t)np + 1)) ||
      (rc = S.err.reserve(c, ROWS_E_COUNT))) return rc;
  const unsigned long long pool_words = B.d_cigar ? B.cigar_words : 0ull;
  RowsSrc src; src.text = B.fx_text; src.n_text = B.fx_n; src.fastq = B.fx_fastq; src.hoff = B.fx_hoff; src.soff = B.fx_soff;
  RowsRef ref; ref.names = di.rows_names; ref.name_off = di.rows_name_off; ref.tab = S.tab;
  const DReads rd = dreads(c);
  const DIndex dx = dindex(di);
  uint32_t h_err[ROWS_E_COUNT];
  for (int attempt = 0;; attempt++) {
    HIPCHK(c, hipMemsetAsync(S.err, 0, sizeof h_err, c->stream));
    HIPCHK(c, hipEventRecord(T.ev[0], c->stream));
    launch(c, k_rows_stat, dim3((uint32_t)std::min<uint64_t>((ntot + 15u) / 16u, (uint64_t)c->n_cu * 32u)), dim3(256), 0, rd, dx, B.slots, (const RState*)B.d_saved,
           (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar, pool_words, D, S.stat, S.err);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(T.ev[1], c->stream));
    HIPCHK(c, hipMemcpyAsync(h_err, S.err, sizeof h_err, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_err[ROWS_E_NOCIG]) {
      set_err(c, "smr_pairwise_part: " + std::to_string(h_err[ROWS_E_NOCIG]) + " alignments of this (index, part) have no CIGAR yet (call smr_traceback first)");
      return SMR_ERR_STATE;
    }
    if (h_err[ROWS_E_BADREF]) { set_err(c, "smr_pairwise_part: " + std::to_string(h_err[ROWS_E_BADREF]) + " alignments with ref_num out of range"); return SMR_ERR_ARG; }
    if (h_err[ROWS_E_PAST]) { set_err(c, "smr_pairwise_part: " + std::to_string(h_err[ROWS_E_PAST]) + " alignments whose CIGAR runs past its read or its reference"); return SMR_ERR_ARG; }
    if (h_err[ROWS_E_NOCOLS]) { set_err(c, "smr_pairwise_part: " + std::to_string(h_err[ROWS_E_NOCOLS]) + " alignments with a CIGAR without columns"); return SMR_ERR_ARG; }
    if (!h_err[ROWS_E_SCORE]) break;
    // a score above match x the longest read (imported state can hold one): the table for every 16-bit score, once
    if (attempt || D.n_tab >= 65536u) { set_err(c, "smr_pairwise_part: a score beyond the e-value table"); return SMR_ERR_ARG; }
    D.n_tab = 65536u;
    if ((rc = rows_table(c, &db, D.n_tab, who))) return rc;
    ref.tab = S.tab;
  }
  float f = 0;
  if (hipEventElapsedTime(&f, T.ev[0], T.ev[1]) == hipSuccess) T.ms[0] = f;
  HIPCHK(c, hipEventRecord(T.ev[2], c->stream));
  launch(c, k_pair_size, dim3(np), dim3(ROWS_BLOCK), 0, rd, dx, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar, pool_words,
         src, ref, D, S.meta, S.excl_b, S.part_b);
  launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.part_b, np + 1u);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(T.ev[3], c->stream));
  unsigned long long total = 0;
  HIPCHK(c, hipMemcpyAsync(&total, S.part_b + np, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (hipEventElapsedTime(&f, T.ev[2], T.ev[3]) == hipSuccess) T.ms[1] = f;
  *need = total;
  if (!bytes) return SMR_OK;
  if (cap < total) { set_err(c, "smr_pairwise_part: the text takes " + std::to_string(total) + " bytes, the buffer has " + std::to_string(cap)); return SMR_ERR_CAPACITY; }
  if (total == 0) return SMR_OK;
  if (S.out.cap() < total + 8u && (rc = S.out.alloc(c, (size_t)((total + (total >> 3) + 4095u) & ~4095ull)))) return rc;      // (the next, slightly larger call fits as well)
  const uint32_t chunks = (n + 63u) / 64u, blocks = std::max(1u, std::min<uint32_t>((chunks + 3u) / 4u, (uint32_t)c->n_cu * 8u));
  HIPCHK(c, hipEventRecord(T.ev[4], c->stream));
  launch(c, k_pair_write, dim3(blocks), dim3(256), 0, rd, dx, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar, pool_words,
         src, ref, D, (const uint4*)S.meta, (const unsigned long long*)S.excl_b, (const unsigned long long*)S.part_b, S.out);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(T.ev[5], c->stream));
  HIPCHK(c, hipMemcpyAsync(bytes, S.out, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(T.ev[6], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (hipEventElapsedTime(&f, T.ev[4], T.ev[5]) == hipSuccess) T.ms[2] = f;
  if (hipEventElapsedTime(&f, T.ev[5], T.ev[6]) == hipSuccess) T.ms[3] = f;
  return SMR_OK;
}

extern "C" int smr_pairwise_times(const smr_ctx* c, double ms[4]) {
  if (!c || !ms) return SMR_ERR_ARG;
  for (int k = 0; k < 4; k++) ms[k] = c->pair.ms[k];
  return SMR_OK;
}
