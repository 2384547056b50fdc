// smr_engine_mates.hpp -- host side of smr_rows_part_mates, smr_pairwise_part_mates and their _gz forms (included by smr_engine.hip behind
// smr_engine_pairwise.hpp; kernel in smr_mates.hpp): the SAM / BLAST rows and the pairwise text of one (index, part) for mates that were read
// from two files -- read i of the selected batch and read i of batch `mates` -- in the order in which smr_report_add_pair appends them.  The
// guard, size and write stages are those of the plain calls (rows_sizes / rows_write, pair_sizes / pair_write), run over the selected batch
// with c->rows and over the mates' batch with c->rows_m; k_mates_zip then interleaves the two staged outputs into c->mates_out from the offsets
// the size kernels left on the device, and that buffer is copied to the host or handed to gz_run exactly where the plain forms hand S.out.
// The e-value table (made for the longer max_len of the two batches) and the slot's reference names are shared.  No call here selects a batch.
//
// Device memory, kept and grown only: what the plain call keeps (c->rows), the same once more for the mates' batch (c->rows_m: stat, meta,
// excl_*, part_*, err, out) and the interleaved output (c->mates_out: the bytes of both batches plus an eighth).  smr_interleave_batch keeps
// its offsets (c->mates_off) and frees its byte buffers when it returns.

namespace {
uint32_t mates_blocks(const smr_ctx* c, uint32_t n) {
  const uint32_t groups = (n + MATES_GROUP - 1u) / MATES_GROUP;
  return std::max(1u, std::min<uint32_t>((groups + 3u) / 4u, (uint32_t)c->n_cu * 8u));
}
// the call's own argument `mates`
int mates_arg(smr_ctx* c, const std::string& W, int mates) {
  if (mates < 0 || mates >= SMR_MAX_BATCHES || &c->bt[mates] == c->b) { set_err(c, W + "`mates` must be a batch 0..15 other than the selected one"); return SMR_ERR_ARG; }
  return SMR_OK;
}
// the refusals of batch `mates` as a batch (behind every refusal of the plain call for the selected batch A)
int mates_open(smr_ctx* c, const std::string& W, int mates, const Batch& A, const Batch& M) {
  if (!M.d_saved || !M.fx_kept) {
    set_err(c, W + "batch " + std::to_string(mates) + " holds no reads, or not their text (upload them with smr_reads_upload_fastx_batch and SMR_FASTX_KEEP)");
    return SMR_ERR_STATE;
  }
  if (M.n != A.n) { set_err(c, W + std::to_string(A.n) + " reads, " + std::to_string(M.n) + " mates"); return SMR_ERR_ARG; }
  if (M.fx_fastq != A.fx_fastq) { set_err(c, W + "FASTA reads with FASTQ mates (or the other way round)"); return SMR_ERR_ARG; }
  return SMR_OK;
}
// ms[0] / ms[1] of smr_mates_times: the stages of one batch, summed
double mates_sum(const StageClock<7, 4>& T) { double t[4]; T.copy_to(t); return t[0] + t[1] + t[2]; }

// c->mates_out (interleaved, `total` bytes staged) -> the host, or through gz_run; behind the interleave kernels (event 1 of the zip clock)
int mates_finish(smr_ctx* c, const char* who, bool wrote_a, bool wrote_m, const uint64_t* off, uint32_t n_streams, uint64_t total, uint8_t* bytes, uint64_t cap,
                 uint64_t* gz_off, uint64_t* need) {
  StageClock<3, 2>& Z = c->mates_zip_clk;
  int rc;
  if (gz_off) {
    if ((rc = gz_run(c, who, c->mates_out, off, n_streams, bytes, cap, gz_off, need, true)) && rc != SMR_ERR_CAPACITY) return rc;
  } else {
    HIPCHK(c, hipMemcpyAsync(bytes, c->mates_out, (size_t)total, hipMemcpyDeviceToHost, c->stream));
    if ((rc = Z.mark(c, 2, c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    Z.set(1, 1, 2);
    rc = SMR_OK;
  }
  if (wrote_a) c->mates_clk[0].set(2, 4, 5);
  if (wrote_m) c->mates_clk[1].set(2, 4, 5);
  Z.set(0, 0, 1);
  return rc;
}

// smr_rows_part_mates (gz_off null) and smr_rows_part_mates_gz: rows_impl over two batches
int rows_mates_impl(smr_ctx* c, const char* who, int mates, int slot, const smr_params* p, const smr_index* ix, const smr_rows_opts* o, uint8_t* bytes, uint64_t cap,
                    uint64_t* off, uint64_t* gz_off, uint64_t* need) {
  const bool zip = gz_off != nullptr;
  const std::string W = std::string(who) + ": ";
  off[0] = off[1] = off[2] = 0;
  if (zip) gz_off[0] = gz_off[1] = gz_off[2] = 0;
  if (need) *need = 0;
  if (!o || !ix || !p || slot < 0 || slot >= 64) { set_err(c, W + "null options, parameters or index, or a slot outside 0..63"); return SMR_ERR_ARG; }
  int rc = mates_arg(c, W, mates); if (rc) return rc;
  RowsOpts D;
  if ((rc = rows_check_opts(c, W, slot, ix, o, D))) return rc;
  Batch& A = *c->b;
  Batch& M = c->bt[mates];
  const std::string who_m = std::string(who) + " (batch " + std::to_string(mates) + ")";
  PartCall pa = {c->idx[slot], A}, pm = {c->idx[slot], M};
  if ((rc = part_call_open(c, who, p, ix, pa))) return rc;
  StageClock<7, 4>&TA = c->mates_clk[0], &TM = c->mates_clk[1];
  StageClock<3, 2>& Z = c->mates_zip_clk;
  if ((rc = TA.begin(c)) || (rc = TM.begin(c)) || (rc = Z.begin(c))) return rc;
  D.want_sam = o->want_sam != 0; D.want_blast = o->want_blast != 0; D.index_num = p->index_num; D.part = p->part;
  RowsRef ref; ref.names = nullptr; ref.name_off = nullptr; ref.tab = nullptr;
  unsigned long long ta[2] = {0, 0}, tm[2] = {0, 0};
  if (A.n) {                                           // the plain call's stages, and with them its refusals, for the selected batch
    if ((rc = part_call_views(c, who, pa))) return rc;
    if ((rc = rows_names(c, pa.di, ix, p->part, who))) return rc;
    if (D.want_blast) {
      D.n_tab = (uint32_t)std::min<uint64_t>(65536u, (uint64_t)p->match * std::max(A.max_len, M.n == A.n ? M.max_len : 0u) + 1u);
      if ((rc = rows_table(c, o, D.n_tab, who))) return rc;
    }
    ref.names = pa.di.rows_names; ref.name_off = pa.di.rows_name_off; ref.tab = c->rows.tab;
    if ((rc = rows_sizes(c, who, TA, pa, c->rows, D, ref, o, ta))) return rc;
  }
  if ((rc = mates_open(c, W, mates, A, M))) return rc;
  if (A.n == 0) return SMR_OK;
  if ((rc = part_call_views(c, who_m.c_str(), pm))) return rc;
  if ((rc = rows_sizes(c, who_m.c_str(), TM, pm, c->rows_m, D, ref, o, tm))) return rc;
  const uint64_t total = ta[0] + ta[1] + tm[0] + tm[1];
  off[1] = ta[0] + tm[0]; off[2] = total;
  if (need) *need = total;
  if (zip) *need = 0;                                  // (until gz_run knows the size of the members)
  else {
    if (!bytes) return SMR_OK;
    if (cap < total) { set_err(c, W + "the rows take " + std::to_string(total) + " bytes, the buffer has " + std::to_string(cap)); return SMR_ERR_CAPACITY; }
  }
  if (total == 0) return SMR_OK;
  const bool wa = ta[0] + ta[1] != 0, wm = tm[0] + tm[1] != 0;
  if (wa && (rc = rows_write(c, TA, pa, c->rows, D, ref, ta))) return rc;
  if (wm && (rc = rows_write(c, TM, pm, c->rows_m, D, ref, tm))) return rc;
  if ((rc = c->mates_out.reserve_headroom(c, (size_t)total, 8))) return rc;
  const RowsScratch &SA = c->rows, &SM = c->rows_m;
  if ((rc = Z.mark(c, 0, c->stream))) return rc;
  if (off[1]) launch(c, k_mates_zip, dim3(mates_blocks(c, pa.n)), dim3(256), 0, pa.n, MatesSrc{SA.out, 0ull, SA.excl_s, SA.part_s}, MatesSrc{SM.out, 0ull, SM.excl_s, SM.part_s}, 0ull,
                     c->mates_out);
  if (total - off[1]) launch(c, k_mates_zip, dim3(mates_blocks(c, pa.n)), dim3(256), 0, pa.n, MatesSrc{SA.out, ta[0], SA.excl_b, SA.part_b}, MatesSrc{SM.out, tm[0], SM.excl_b, SM.part_b},
                             (unsigned long long)off[1], c->mates_out);
  HIPCHK(c, hipGetLastError());
  if ((rc = Z.mark(c, 1, c->stream))) return rc;
  return mates_finish(c, who, wa, wm, off, 2, total, bytes, cap, gz_off, need);
}

// smr_pairwise_part_mates (plain_bytes null) and smr_pairwise_part_mates_gz: pair_impl over two batches
int pair_mates_impl(smr_ctx* c, const char* who, int mates, int slot, const smr_params* p, const smr_index* ix, double lambda, double K, uint64_t full_ref_corr,
                    uint64_t full_read_corr, uint8_t* bytes, uint64_t cap, uint64_t* plain_bytes, uint64_t* need) {
  const bool zip = plain_bytes != nullptr;
  const std::string W = std::string(who) + ": ";
  *need = 0;
  if (zip) *plain_bytes = 0;
  if (!ix || !p || slot < 0 || slot >= 64) { set_err(c, W + "null parameters or index, or a slot outside 0..63"); return SMR_ERR_ARG; }
  int rc = mates_arg(c, W, mates); if (rc) return rc;
  Batch& A = *c->b;
  Batch& M = c->bt[mates];
  const std::string who_m = std::string(who) + " (batch " + std::to_string(mates) + ")";
  PartCall pa = {c->idx[slot], A}, pm = {c->idx[slot], M};
  if ((rc = part_call_open(c, who, p, ix, pa))) return rc;
  StageClock<7, 4>&TA = c->mates_clk[0], &TM = c->mates_clk[1];
  StageClock<3, 2>& Z = c->mates_zip_clk;
  if ((rc = TA.begin(c)) || (rc = TM.begin(c)) || (rc = Z.begin(c))) return rc;
  RowsOpts D;
  memset(&D, 0, sizeof D);
  D.want_blast = 1; D.index_num = p->index_num; D.part = p->part;       // (want_blast: k_rows_stat checks the scores against the table)
  smr_rows_opts db;
  memset(&db, 0, sizeof db);
  db.lambda = lambda; db.K = K; db.full_ref_corr = full_ref_corr; db.full_read_corr = full_read_corr;
  RowsRef ref; ref.names = nullptr; ref.name_off = nullptr; ref.tab = nullptr;
  unsigned long long ta = 0, tm = 0;
  if (A.n) {                                           // the plain call's stages, and with them its refusals, for the selected batch
    if ((rc = part_call_views(c, who, pa))) return rc;
    if ((rc = rows_names(c, pa.di, ix, p->part, who))) return rc;
    D.n_tab = (uint32_t)std::min<uint64_t>(65536u, (uint64_t)p->match * std::max(A.max_len, M.n == A.n ? M.max_len : 0u) + 1u);
    if ((rc = rows_table(c, &db, D.n_tab, who))) return rc;
    ref.names = pa.di.rows_names; ref.name_off = pa.di.rows_name_off; ref.tab = c->rows.tab;
    if ((rc = pair_sizes(c, who, TA, pa, c->rows, D, ref, &db, &ta))) return rc;
  }
  if ((rc = mates_open(c, W, mates, A, M))) return rc;
  if (A.n == 0) return SMR_OK;
  if ((rc = part_call_views(c, who_m.c_str(), pm))) return rc;
  if ((rc = pair_sizes(c, who_m.c_str(), TM, pm, c->rows_m, D, ref, &db, &tm))) return rc;
  const uint64_t total = ta + tm;
  if (zip) *plain_bytes = total;                      // (*need stays 0 until gz_run knows the size of the members)
  else {
    *need = total;
    if (!bytes) return SMR_OK;
    if (cap < total) { set_err(c, W + "the text takes " + std::to_string(total) + " bytes, the buffer has " + std::to_string(cap)); return SMR_ERR_CAPACITY; }
  }
  if (total == 0) return SMR_OK;
  if (ta && (rc = pair_write(c, TA, pa, c->rows, D, ref, ta))) return rc;
  if (tm && (rc = pair_write(c, TM, pm, c->rows_m, D, ref, tm))) return rc;
  if ((rc = c->mates_out.reserve_headroom(c, (size_t)total, 8))) return rc;
  const RowsScratch &SA = c->rows, &SM = c->rows_m;
  if ((rc = Z.mark(c, 0, c->stream))) return rc;
  launch(c, k_mates_zip, dim3(mates_blocks(c, pa.n)), dim3(256), 0, pa.n, MatesSrc{SA.out, 0ull, SA.excl_b, SA.part_b}, MatesSrc{SM.out, 0ull, SM.excl_b, SM.part_b}, 0ull, c->mates_out);
  HIPCHK(c, hipGetLastError());
  if ((rc = Z.mark(c, 1, c->stream))) return rc;
  const uint64_t off[2] = {0, total};
  uint64_t gz_off[2];
  return mates_finish(c, who, ta != 0, tm != 0, off, 1, total, bytes, cap, zip ? gz_off : nullptr, need);
}
}  // namespace

extern "C" int smr_rows_part_mates(smr_ctx* c, int mates, int slot, const smr_params* p, const smr_index* ix, const smr_rows_opts* o,
                                   uint8_t* bytes, uint64_t cap, uint64_t off[3], uint64_t* need) {
  if (!c || !off) return SMR_ERR_ARG;
  return rows_mates_impl(c, "smr_rows_part_mates", mates, slot, p, ix, o, bytes, cap, off, nullptr, need);
}
extern "C" int smr_rows_part_mates_gz(smr_ctx* c, int mates, int slot, const smr_params* p, const smr_index* ix, const smr_rows_opts* o,
                                      uint8_t* gz, uint64_t cap, uint64_t gz_off[3], uint64_t plain_off[3], uint64_t* need) {
  if (!c || !gz_off || !plain_off || !need) return SMR_ERR_ARG;
  return rows_mates_impl(c, "smr_rows_part_mates_gz", mates, slot, p, ix, o, gz, cap, plain_off, gz_off, need);
}
extern "C" int smr_pairwise_part_mates(smr_ctx* c, int mates, int slot, const smr_params* p, const smr_index* ix, double lambda, double K, uint64_t full_ref_corr,
                                       uint64_t full_read_corr, uint8_t* bytes, uint64_t cap, uint64_t* need) {
  if (!c || !need) return SMR_ERR_ARG;
  return pair_mates_impl(c, "smr_pairwise_part_mates", mates, slot, p, ix, lambda, K, full_ref_corr, full_read_corr, bytes, cap, nullptr, need);
}
extern "C" int smr_pairwise_part_mates_gz(smr_ctx* c, int mates, int slot, const smr_params* p, const smr_index* ix, double lambda, double K, uint64_t full_ref_corr,
                                          uint64_t full_read_corr, uint8_t* gz, uint64_t cap, uint64_t* plain_bytes, uint64_t* need) {
  if (!c || !plain_bytes || !need) return SMR_ERR_ARG;
  return pair_mates_impl(c, "smr_pairwise_part_mates_gz", mates, slot, p, ix, lambda, K, full_ref_corr, full_read_corr, gz, cap, plain_bytes, need);
}

extern "C" int smr_mates_times(const smr_ctx* c, double ms[4]) {
  if (!c || !ms) return SMR_ERR_ARG;
  double z[2];
  c->mates_zip_clk.copy_to(z);
  ms[0] = mates_sum(c->mates_clk[0]); ms[1] = mates_sum(c->mates_clk[1]); ms[2] = z[0]; ms[3] = z[1];
  return SMR_OK;
}

// k_mates_zip at its seam: pieces from the host, the offsets brought into the form the size kernels leave (excl[i] within a block of ROWS_BLOCK
// pieces, part[b] in front of block b, part[np] the total), the interleaved bytes back
extern "C" int smr_interleave_batch(smr_ctx* c, uint32_t n, const uint8_t* a, const uint64_t* a_off, const uint8_t* b, const uint64_t* b_off, uint8_t* out, uint64_t cap,
                                    uint64_t* need) {
  if (!c || !need) return SMR_ERR_ARG;
  *need = 0;
  if (n == 0) return SMR_OK;
  if (!a_off || !b_off) { set_err(c, "smr_interleave_batch: null offsets"); return SMR_ERR_ARG; }
  for (uint32_t i = 0; i < n; i++) if (a_off[i + 1] < a_off[i] || b_off[i + 1] < b_off[i]) { set_err(c, "smr_interleave_batch: the offsets decrease"); return SMR_ERR_ARG; }
  const uint64_t la = a_off[n] - a_off[0], lb = b_off[n] - b_off[0], total = la + lb;
  if ((la && !a) || (lb && !b)) { set_err(c, "smr_interleave_batch: null pieces"); return SMR_ERR_ARG; }
  *need = total;
  if (!out) return SMR_OK;
  if (cap < total) { set_err(c, "smr_interleave_batch: the pieces take " + std::to_string(total) + " bytes, the buffer has " + std::to_string(cap)); return SMR_ERR_CAPACITY; }
  if (total == 0) return SMR_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const uint32_t np = (n + ROWS_BLOCK - 1u) / ROWS_BLOCK;
  std::vector<unsigned long long> h(2 * ((size_t)n + np + 1u));
  unsigned long long* const ea = h.data(), *const eb = ea + n, *const pa = eb + n, *const pb = pa + np + 1u;
  for (uint32_t i = 0; i < n; i++) {
    if (i % ROWS_BLOCK == 0u) { pa[i / ROWS_BLOCK] = a_off[i] - a_off[0]; pb[i / ROWS_BLOCK] = b_off[i] - b_off[0]; }
    ea[i] = a_off[i] - a_off[0] - pa[i / ROWS_BLOCK]; eb[i] = b_off[i] - b_off[0] - pb[i / ROWS_BLOCK];
  }
  pa[np] = la; pb[np] = lb;
  DevBuf<uint8_t> d_a, d_b, d_out;                      // (the sources padded by 8, the output exact: the kernel stores nothing behind it)
  int rc;
  if ((rc = d_a.alloc(c, (size_t)la + 8u)) || (rc = d_b.alloc(c, (size_t)lb + 8u)) || (rc = d_out.alloc(c, (size_t)total)) || (rc = c->mates_off.reserve(c, h.size()))) return rc;
  if (la) HIPCHK(c, hipMemcpyAsync(d_a, a + a_off[0], (size_t)la, hipMemcpyHostToDevice, c->stream));
  if (lb) HIPCHK(c, hipMemcpyAsync(d_b, b + b_off[0], (size_t)lb, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(c->mates_off, h.data(), h.size() * 8u, hipMemcpyHostToDevice, c->stream));
  const unsigned long long* const d = c->mates_off;
  launch(c, k_mates_zip, dim3(mates_blocks(c, n)), dim3(256), 0, n, MatesSrc{d_a, 0ull, d, d + 2 * (size_t)n}, MatesSrc{d_b, 0ull, d + n, d + 2 * (size_t)n + np + 1u}, 0ull, d_out);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, d_out, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SMR_OK;
}
