// smr_engine_pairwise.hpp -- host side of smr_pairwise_part (included by smr_engine.hip behind smr_engine_rows.hpp; kernels in smr_pairwise.hpp):
// the BLAST-like pairwise text (-blast 0) of one (index, part) over the selected batch, guarded, sized and written on the device -- what
// smr_results_fetch + smr_reads_record_text + smr_result_record + smr_report_add do on the host one read at a time.  The host's share is that of
// smr_rows_part, whose pieces are used as they are: the preamble of a per-part call (PartCall), the names of the part's references (rows_names),
// the e-value / bit-score texts per score (rows_table), the guards of k_rows_stat (rows_guard), the device buffers of RowsScratch; two small
// copies back (the error counts, the total) and the bytes -- or, for smr_pairwise_part_gz, the gzip members that gz_run makes of the text where
// it lies.  Its times are its own (smr_ctx::pair_clk).

namespace {
// The stages of smr_pairwise_part for one batch and its scratch {pc, S} -- the selected batch and c->rows for the plain calls, either batch of a
// pair for the mates' forms (smr_engine_mates.hpp).  pair_sizes: the guards and the sizes (events 0 .. 3 of T, times 0 and 1); pair_write: the
// text into S.out (events 4 and 5 of T)
int pair_sizes(smr_ctx* c, const char* who, StageClock<7, 4>& T, const PartCall& pc, RowsScratch& S, RowsOpts& D, RowsRef& ref, const smr_rows_opts* db, unsigned long long* total) {
  const Batch& B = pc.B;
  const uint32_t n = pc.n, np = (n + ROWS_BLOCK - 1u) / ROWS_BLOCK;
  int rc;
  *total = 0;
  if ((rc = S.stat.reserve(c, pc.ntot)) || (rc = S.meta.reserve(c, n)) || (rc = S.excl_b.reserve(c, n)) || (rc = S.part_b.reserve(c, (size_t)np + 1)) ||
      (rc = S.err.reserve(c, ROWS_E_COUNT))) return rc;
  if ((rc = rows_guard(c, who, T, pc, S, D, ref, db))) return rc;
  if ((rc = T.mark(c, 2, c->stream))) return rc;
  launch(c, k_pair_size, dim3(np), dim3(ROWS_BLOCK), 0, pc.rd, pc.dx, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar, pc.pool_words,
         pc.src, ref, D, S.meta, S.excl_b, S.part_b);
  launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.part_b, np + 1u);
  HIPCHK(c, hipGetLastError());
  if ((rc = T.mark(c, 3, c->stream))) return rc;
  HIPCHK(c, hipMemcpyAsync(total, S.part_b + np, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  T.set(1, 2, 3);
  return SMR_OK;
}
int pair_write(smr_ctx* c, StageClock<7, 4>& T, const PartCall& pc, RowsScratch& S, const RowsOpts& D, const RowsRef& ref, unsigned long long total) {
  const Batch& B = pc.B;
  const uint32_t n = pc.n;
  int rc;
  if ((rc = S.out.reserve_headroom(c, (size_t)total, 8))) return rc;
  const uint32_t chunks = (n + 63u) / 64u, blocks = std::max(1u, std::min<uint32_t>((chunks + 3u) / 4u, (uint32_t)c->n_cu * 8u));
  if ((rc = T.mark(c, 4, c->stream))) return rc;
  launch(c, k_pair_write, dim3(blocks), dim3(256), 0, pc.rd, pc.dx, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar, pc.pool_words,
         pc.src, ref, D, (const uint4*)S.meta, (const unsigned long long*)S.excl_b, (const unsigned long long*)S.part_b, S.out);
  HIPCHK(c, hipGetLastError());
  return T.mark(c, 5, c->stream);
}

// The writer behind smr_pairwise_part (plain_bytes null: `bytes` takes the text, *need its size) and smr_pairwise_part_gz (plain_bytes given:
// the text stays on the device and goes through gz_run with cuts at line ends, `bytes` takes the gzip members, *need their size, *plain_bytes
// what the plain call returns)
int pair_impl(smr_ctx* c, const char* who, int slot, const smr_params* p, const smr_index* ix, double lambda, double K, uint64_t full_ref_corr, uint64_t full_read_corr,
              uint8_t* bytes, uint64_t cap, uint64_t* plain_bytes, uint64_t* need) {
  const bool zip = plain_bytes != nullptr;
  const std::string W = std::string(who) + ": ";
  *need = 0;
  if (zip) *plain_bytes = 0;
  if (!ix || slot < 0 || slot >= 64) { set_err(c, W + "null index, or a slot outside 0..63"); return SMR_ERR_ARG; }
  PartCall pc = {c->idx[slot], *c->b};
  int rc = part_call_open(c, who, p, ix, pc); if (rc) return rc;
  const Batch& B = pc.B;
  if (B.n == 0) return SMR_OK;
  if ((rc = part_call_views(c, who, pc))) return rc;
  RowsOpts D;
  memset(&D, 0, sizeof D);
  D.want_blast = 1; D.index_num = p->index_num; D.part = p->part;       // (want_blast: k_rows_stat checks the scores against the table)
  smr_rows_opts db;
  memset(&db, 0, sizeof db);
  db.lambda = lambda; db.K = K; db.full_ref_corr = full_ref_corr; db.full_read_corr = full_read_corr;
  RowsScratch& S = c->rows;
  StageClock<7, 4>& T = c->pair_clk;
  if ((rc = T.begin(c))) return rc;
  if ((rc = rows_names(c, pc.di, ix, p->part, who))) return rc;
  D.n_tab = (uint32_t)std::min<uint64_t>(65536u, (uint64_t)p->match * B.max_len + 1u);
  if ((rc = rows_table(c, &db, D.n_tab, who))) return rc;
  RowsRef ref; ref.names = pc.di.rows_names; ref.name_off = pc.di.rows_name_off; ref.tab = S.tab;
  unsigned long long total = 0;
  if ((rc = pair_sizes(c, who, T, pc, S, D, ref, &db, &total))) return rc;
  if (zip) *plain_bytes = total;                      // (*need stays 0 until gz_run knows the size of the members)
  else {
    *need = total;
    if (!bytes) return SMR_OK;
    if (cap < total) { set_err(c, W + "the text takes " + std::to_string(total) + " bytes, the buffer has " + std::to_string(cap)); return SMR_ERR_CAPACITY; }
  }
  if (total == 0) return SMR_OK;
  if ((rc = pair_write(c, T, pc, S, D, ref, total))) return rc;
  if (zip) {                                           // (the time of a copy that is not made stays 0)
    const uint64_t off[2] = {0, total};
    uint64_t gz_off[2];
    if ((rc = gz_run(c, who, S.out, off, 1, bytes, cap, gz_off, need, true)) && rc != SMR_ERR_CAPACITY) return rc;
    T.set(2, 4, 5);
    return rc;
  }
  HIPCHK(c, hipMemcpyAsync(bytes, S.out, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  if ((rc = T.mark(c, 6, c->stream))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  T.set(2, 4, 5);
  T.set(3, 5, 6);
  return SMR_OK;
}
}  // namespace

extern "C" int smr_pairwise_part(smr_ctx* c, int slot, const smr_params* p, const smr_index* ix, double lambda, double K, uint64_t full_ref_corr,
                                 uint64_t full_read_corr, uint8_t* bytes, uint64_t cap, uint64_t* need) {
  if (!c || !need) return SMR_ERR_ARG;
  return pair_impl(c, "smr_pairwise_part", slot, p, ix, lambda, K, full_ref_corr, full_read_corr, bytes, cap, nullptr, need);
}
extern "C" int smr_pairwise_part_gz(smr_ctx* c, int slot, const smr_params* p, const smr_index* ix, double lambda, double K, uint64_t full_ref_corr,
                                    uint64_t full_read_corr, uint8_t* gz, uint64_t cap, uint64_t* plain_bytes, uint64_t* need) {
  if (!c || !plain_bytes || !need) return SMR_ERR_ARG;
  return pair_impl(c, "smr_pairwise_part_gz", slot, p, ix, lambda, K, full_ref_corr, full_read_corr, gz, cap, plain_bytes, need);
}

extern "C" int smr_pairwise_times(const smr_ctx* c, double ms[4]) {
  if (!c || !ms) return SMR_ERR_ARG;
  c->pair_clk.copy_to(ms);
  return SMR_OK;
}
