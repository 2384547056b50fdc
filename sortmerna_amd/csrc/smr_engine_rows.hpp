// smr_engine_rows.hpp -- host side of smr_rows_part (included by smr_engine.hip; kernels in smr_rows.hpp): the rows of aligned.sam and of the
// BLAST tabular report of one (index, part) over the selected batch, counted, sized and written on the device -- what smr_results_fetch +
// smr_reads_record_text + smr_result_record + smr_report_add do on the host one read at a time.  The host's share: the names of the part's
// references (uploaded once per slot), the e-value / bit-score texts per score (smr::score_texts, the report writer's own), three small
// copies back (the error counts, the two totals) and the bytes -- or, for smr_rows_part_gz, the gzip members that gz_run (smr_engine_gzip.hpp)
// makes of the rows where they lie.  Also here, for smr_pairwise_part and smr_otu_part behind it: the preamble of a
// call on one (index, part) (PartCall, part_call_open, part_call_views) and the guard loop of k_rows_stat (rows_guard).

namespace {
// blast_cols -> ROWS_COL_*; false for an unknown word
bool rows_parse_cols(const char* text, RowsOpts& D) {
  D.ncols = 0; D.cols = 0;
  char buf[65]; memcpy(buf, text, 64); buf[64] = 0;
  for (const char* p = buf; *p;) {
    const char* e = strchr(p, ' ');
    const std::string col = e ? std::string(p, e) : std::string(p);
    if (!col.empty()) {
      uint32_t id = col == "cigar" ? ROWS_COL_CIGAR : col == "qcov" ? ROWS_COL_QCOV : col == "qstrand" ? ROWS_COL_QSTRAND : 0u;
      if (!id || D.ncols >= ROWS_MAX_COLS) return false;      // (a word may come twice, as with the host writer; 64 characters hold no more than twelve)
      D.cols |= id << (2u * D.ncols++);
    }
    p = e ? e + 1 : p + col.size();
  }
  return true;
}

// the names of the references of part `part` as the rows print them: sq_header[first_seq + ref_num].first, "*" beyond the table
int rows_names(smr_ctx* c, DevIndex& d, const smr_index* ix, uint32_t part, const char* who) {
  if (d.rows_names && d.rows_part == (int64_t)part) return SMR_OK;
  size_t first_seq = 0;
  for (uint32_t q = 0; q < part && q < ix->parts.size(); q++) first_seq += ix->parts[q].numseq_part;
  std::vector<uint32_t> off((size_t)d.n_refs + 1);
  std::string all;
  for (uint32_t r = 0; r < d.n_refs; r++) {
    off[r] = (uint32_t)all.size();
    if (first_seq + r < ix->sq_header.size()) all += ix->sq_header[first_seq + r].first; else all += '*';
    if (all.size() >= 0xFFFFFF00ull) { set_err(c, std::string(who) + ": the reference names of the part take 4 GiB or more"); return SMR_ERR_CAPACITY; }
  }
  off[d.n_refs] = (uint32_t)all.size();
  all.resize((all.size() + 8u) & ~(size_t)3u, '\0');     // (the kernels fetch a byte as part of its aligned dword)
  int rc;
  d.rows_part = -1;
  if ((rc = d.rows_names.alloc(c, all.size())) || (rc = d.rows_name_off.alloc(c, off.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(d.rows_names, all.data(), all.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d.rows_name_off, off.data(), off.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  d.rows_part = (int64_t)part;
  return SMR_OK;
}

// the texts of e-value and bit score for score1 = 0 .. n_tab - 1 under the database of `o`; kept until another database or a higher score asks
int rows_table(smr_ctx* c, const smr_rows_opts* o, uint32_t n_tab, const char* who) {
  RowsScratch& S = c->rows;
  if (S.tab && S.tab_n >= n_tab && S.tab_lambda == o->lambda && S.tab_K == o->K && S.tab_ref == o->full_ref_corr && S.tab_read == o->full_read_corr) return SMR_OK;
  std::vector<uint8_t> h((size_t)n_tab * ROWS_TAB_ENTRY, 0);
  std::string ev, bs;
  for (uint32_t s = 0; s < n_tab; s++) {
    score_texts(o->lambda, o->K, o->full_ref_corr, o->full_read_corr, s, ev, bs);
    if (ev.size() > 14u || bs.size() > 16u) { set_err(c, std::string(who) + ": an e-value or bit score of more than 14 / 16 characters"); return SMR_ERR_ARG; }
    uint8_t* e = h.data() + (size_t)s * ROWS_TAB_ENTRY;
    e[0] = (uint8_t)ev.size(); e[1] = (uint8_t)bs.size();
    memcpy(e + 2, ev.data(), ev.size()); memcpy(e + 16, bs.data(), bs.size());
  }
  int rc;
  S.tab_n = 0;
  if ((rc = S.tab.reserve(c, h.size()))) return rc;
  HIPCHK(c, hipMemcpyAsync(S.tab, h.data(), h.size(), hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  S.tab_n = n_tab; S.tab_lambda = o->lambda; S.tab_K = o->K; S.tab_ref = o->full_ref_corr; S.tab_read = o->full_read_corr;
  return SMR_OK;
}

// ---- what smr_rows_part, smr_pairwise_part and smr_otu_part share: the checks of a call on (the part in `slot`, the selected batch) and what its
// kernels are handed of the two
struct PartCall {
  DevIndex& di; Batch& B;
  uint64_t ntot; uint32_t n; unsigned long long pool_words;      // reads x alignment slots, reads, words of the CIGAR pool
  RowsSrc src; DReads rd; DIndex dx;
};
// the refusals, in the order in which they take precedence, of a call made as {c->idx[slot], *c->b}; the caller has checked its own arguments
// (slot within 0..63 among them).  The mates' forms (smr_engine_mates.hpp) make it for the selected batch as well: no call here looks at c->b
int part_call_open(smr_ctx* c, const char* who, const smr_params* p, const smr_index* ix, const PartCall& pc) {
  const std::string W = std::string(who) + ": ";
  if (!pc.di.used || !pc.B.d_saved) { set_err(c, W + "index slot empty or no reads uploaded"); return SMR_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  int rc = check_params(c, p, false); if (rc) return rc;
  if (pc.di.n_refs != ix->n_refs() || pc.di.ref_bytes != ix->ref_seq.size() || pc.di.lnwin != ix->lnwin) { set_err(c, W + "`ix` is not the index part that is resident in the slot"); return SMR_ERR_ARG; }
  if (!pc.B.fx_kept) { set_err(c, W + "the batch does not hold its text (upload it with smr_reads_upload_fastx* and SMR_FASTX_KEEP)"); return SMR_ERR_STATE; }
  return SMR_OK;
}
// behind the caller's early return (a batch with reads): the size limit, then the views
int part_call_views(smr_ctx* c, const char* who, PartCall& pc) {
  const Batch& B = pc.B;
  pc.n = B.n; pc.ntot = (uint64_t)B.n * B.slots;
  if (pc.ntot >= 0xFFFFFC00ull) { set_err(c, std::string(who) + ": reads x alignment slots of the batch must stay below 2^32"); return SMR_ERR_CAPACITY; }
  pc.pool_words = B.d_cigar ? B.cigar_words : 0ull;
  pc.src.text = B.fx_text; pc.src.n_text = B.fx_n; pc.src.fastq = B.fx_fastq; pc.src.hoff = B.fx_hoff; pc.src.soff = B.fx_soff;
  pc.rd = dreads(pc.B); pc.dx = dindex(pc.di);
  return SMR_OK;
}
// k_rows_stat over the batch (events 0 and 1 of `clk`, time 0): the statistics of every alignment, and the refusal of state the writers would
// read out of bounds for.  A score above the table of D.n_tab entries makes the table for every 16-bit score under `db`, once.  S: the scratch of
// the batch (stat, err); the table is that of c->rows whichever batch asks
int rows_guard(smr_ctx* c, const char* who, StageClock<7, 4>& clk, const PartCall& pc, RowsScratch& S, RowsOpts& D, RowsRef& ref, const smr_rows_opts* db) {
  const Batch& B = pc.B;
  const std::string W = std::string(who) + ": ";
  uint32_t h_err[ROWS_E_COUNT];
  int rc;
  for (int attempt = 0;; attempt++) {
    HIPCHK(c, hipMemsetAsync(S.err, 0, sizeof h_err, c->stream));
    if ((rc = clk.mark(c, 0, c->stream))) return rc;
    launch(c, k_rows_stat, dim3((uint32_t)std::min<uint64_t>((pc.ntot + 15u) / 16u, (uint64_t)c->n_cu * 32u)), dim3(256), 0, pc.rd, pc.dx, B.slots, (const RState*)B.d_saved,
           (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar, pc.pool_words, D, S.stat, S.err);
    HIPCHK(c, hipGetLastError());
    if ((rc = clk.mark(c, 1, c->stream))) return rc;
    HIPCHK(c, hipMemcpyAsync(h_err, S.err, sizeof h_err, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = part_refuse_state(c, who, h_err[ROWS_E_NOCIG], h_err[ROWS_E_BADREF], h_err[ROWS_E_PAST]))) return rc;
    if (h_err[ROWS_E_NOCOLS]) { set_err(c, W + std::to_string(h_err[ROWS_E_NOCOLS]) + " alignments with a CIGAR without columns"); return SMR_ERR_ARG; }
    if (!h_err[ROWS_E_SCORE]) break;
    // a score above match x the longest read (imported state can hold one): the table for every 16-bit score, once
    if (attempt || D.n_tab >= 65536u) { set_err(c, W + "a score beyond the e-value table"); return SMR_ERR_ARG; }
    D.n_tab = 65536u;
    if ((rc = rows_table(c, db, D.n_tab, who))) return rc;
    ref.tab = c->rows.tab;
  }
  clk.set(0, 0, 1);
  return SMR_OK;
}
}  // namespace

namespace {
// The stages of smr_rows_part for one batch and its scratch {pc, S} -- the selected batch and c->rows for the plain calls, either batch of a pair
// for the mates' forms (smr_engine_mates.hpp).  rows_sizes: the guards and the sizes (events 0 .. 3 of T, times 0 and 1); tot[0] / tot[1]: the
// bytes of the SAM / the BLAST rows.  rows_write: the rows into S.out as [SAM | BLAST] (events 4 and 5 of T)
int rows_sizes(smr_ctx* c, const char* who, StageClock<7, 4>& T, const PartCall& pc, RowsScratch& S, RowsOpts& D, RowsRef& ref, const smr_rows_opts* o, unsigned long long tot[2]) {
  const Batch& B = pc.B;
  const uint32_t n = pc.n, np = (n + ROWS_BLOCK - 1u) / ROWS_BLOCK;
  int rc;
  tot[0] = tot[1] = 0;
  if ((rc = S.stat.reserve(c, pc.ntot)) || (rc = S.meta.reserve(c, n)) || (rc = S.excl_s.reserve(c, n)) || (rc = S.excl_b.reserve(c, n)) ||
      (rc = S.part_s.reserve(c, (size_t)np + 1)) || (rc = S.part_b.reserve(c, (size_t)np + 1)) || (rc = S.err.reserve(c, ROWS_E_COUNT))) return rc;
  if ((rc = rows_guard(c, who, T, pc, S, D, ref, o))) return rc;
  if ((rc = T.mark(c, 2, c->stream))) return rc;
  launch(c, k_rows_size, dim3(np), dim3(ROWS_BLOCK), 0, pc.rd, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar, pc.pool_words,
         (const uint4*)S.stat, pc.src, ref, D, S.meta, S.excl_s, S.excl_b, S.part_s, S.part_b);
  launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.part_s, np + 1u);
  launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.part_b, np + 1u);
  HIPCHK(c, hipGetLastError());
  if ((rc = T.mark(c, 3, c->stream))) return rc;
  HIPCHK(c, hipMemcpyAsync(&tot[0], S.part_s + np, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipMemcpyAsync(&tot[1], S.part_b + np, 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  T.set(1, 2, 3);
  return SMR_OK;
}
int rows_write(smr_ctx* c, StageClock<7, 4>& T, const PartCall& pc, RowsScratch& S, const RowsOpts& D, const RowsRef& ref, const unsigned long long tot[2]) {
  const Batch& B = pc.B;
  const uint32_t n = pc.n;
  int rc;
  // the rows, staged on the device: copied to the host from there, or compressed from there
  if ((rc = S.out.reserve_headroom(c, (size_t)(tot[0] + tot[1]), 8))) return rc;
  const uint32_t chunks = (n + 63u) / 64u, blocks = std::max(1u, std::min<uint32_t>((chunks + 3u) / 4u, (uint32_t)c->n_cu * 8u));
  if ((rc = T.mark(c, 4, c->stream))) return rc;
  if (tot[0]) launch(c, k_rows_write<0u>, dim3(blocks), dim3(256), 0, pc.rd, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar, pc.pool_words,
                     (const uint4*)S.stat, pc.src, ref, D, (const uint4*)S.meta, (const unsigned long long*)S.excl_s, (const unsigned long long*)S.part_s, 0ull, S.out);
  if (tot[1]) launch(c, k_rows_write<1u>, dim3(blocks), dim3(256), 0, pc.rd, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar, pc.pool_words,
                     (const uint4*)S.stat, pc.src, ref, D, (const uint4*)S.meta, (const unsigned long long*)S.excl_b, (const unsigned long long*)S.part_b, tot[0], S.out);
  HIPCHK(c, hipGetLastError());
  return T.mark(c, 5, c->stream);
}
// the arguments of smr_rows_part* that are checked before any state: D takes the columns
int rows_check_opts(smr_ctx* c, const std::string& W, int slot, const smr_index* ix, const smr_rows_opts* o, RowsOpts& D) {
  if (!o || !ix || slot < 0 || slot >= 64) { set_err(c, W + "null options or index, or a slot outside 0..63"); return SMR_ERR_ARG; }
  if (!o->want_sam && !o->want_blast) { set_err(c, W + "neither the SAM nor the BLAST rows are wanted"); return SMR_ERR_ARG; }
  memset(&D, 0, sizeof D);
  if (!rows_parse_cols(o->blast_cols, D)) { set_err(c, W + "blast_cols takes \"cigar\", \"qcov\" and \"qstrand\", space separated"); return SMR_ERR_ARG; }
  return SMR_OK;
}

// The writer behind smr_rows_part (gz_off null: `bytes` takes the two streams, `off` their offsets) and smr_rows_part_gz (gz_off given: the
// streams stay on the device and go through gz_run with cuts at line ends, `bytes` takes the gzip members, gz_off their offsets, `off` what
// the plain call returns)
int rows_impl(smr_ctx* c, const char* who, int slot, const smr_params* p, const smr_index* ix, const smr_rows_opts* o, uint8_t* bytes, uint64_t cap, uint64_t* off,
              uint64_t* gz_off, uint64_t* need) {
  const bool zip = gz_off != nullptr;
  const std::string W = std::string(who) + ": ";
  off[0] = off[1] = off[2] = 0;
  if (zip) gz_off[0] = gz_off[1] = gz_off[2] = 0;
  if (need) *need = 0;
  RowsOpts D;
  int rc = rows_check_opts(c, W, slot, ix, o, D); if (rc) return rc;
  PartCall pc = {c->idx[slot], *c->b};
  if ((rc = part_call_open(c, who, p, ix, pc))) return rc;
  const Batch& B = pc.B;
  if (B.n == 0) return SMR_OK;
  if ((rc = part_call_views(c, who, pc))) return rc;
  D.want_sam = o->want_sam != 0; D.want_blast = o->want_blast != 0; D.index_num = p->index_num; D.part = p->part;
  RowsScratch& S = c->rows;
  StageClock<7, 4>& T = S.clk;
  if ((rc = T.begin(c))) return rc;
  if ((rc = rows_names(c, pc.di, ix, p->part, who))) return rc;
  if (D.want_blast) {
    D.n_tab = (uint32_t)std::min<uint64_t>(65536u, (uint64_t)p->match * B.max_len + 1u);
    if ((rc = rows_table(c, o, D.n_tab, who))) return rc;
  }
  RowsRef ref; ref.names = pc.di.rows_names; ref.name_off = pc.di.rows_name_off; ref.tab = S.tab;
  unsigned long long tot[2];
  if ((rc = rows_sizes(c, who, T, pc, S, D, ref, o, tot))) return rc;
  const uint64_t total = tot[0] + tot[1];
  off[1] = tot[0]; off[2] = total;
  if (need) *need = total;
  if (zip) *need = 0;                                  // (until gz_run knows the size of the members)
  else {
    if (!bytes) return SMR_OK;
    if (cap < total) { set_err(c, W + "the rows take " + std::to_string(total) + " bytes, the buffer has " + std::to_string(cap)); return SMR_ERR_CAPACITY; }
  }
  if (total == 0) return SMR_OK;
  if ((rc = rows_write(c, T, pc, S, D, ref, tot))) return rc;
  if (zip) {                                           // (the time of a copy that is not made stays 0)
    if ((rc = gz_run(c, who, S.out, off, 2, bytes, cap, gz_off, need, true)) && rc != SMR_ERR_CAPACITY) return rc;
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

extern "C" int smr_rows_part(smr_ctx* c, int slot, const smr_params* p, const smr_index* ix, const smr_rows_opts* o,
                             uint8_t* bytes, uint64_t cap, uint64_t off[3], uint64_t* need) {
  if (!c || !off) return SMR_ERR_ARG;
  return rows_impl(c, "smr_rows_part", slot, p, ix, o, bytes, cap, off, nullptr, need);
}
extern "C" int smr_rows_part_gz(smr_ctx* c, int slot, const smr_params* p, const smr_index* ix, const smr_rows_opts* o,
                                uint8_t* gz, uint64_t cap, uint64_t gz_off[3], uint64_t plain_off[3], uint64_t* need) {
  if (!c || !gz_off || !plain_off || !need) return SMR_ERR_ARG;
  return rows_impl(c, "smr_rows_part_gz", slot, p, ix, o, gz, cap, plain_off, gz_off, need);
}

extern "C" int smr_rows_times(const smr_ctx* c, double ms[4]) {
  if (!c || !ms) return SMR_ERR_ARG;
  c->rows.clk.copy_to(ms);
  return SMR_OK;
}

// the device formatter at its seam: out[16 i ..] = the text of `stream << (double)num[i] / (double)den[i] * 100` at precision 3, NUL padded
extern "C" int smr_rows_fmt_batch(smr_ctx* c, uint32_t n, const uint32_t* num, const uint32_t* den, char* out) {
  if (!c) return SMR_ERR_ARG;
  if (n == 0) return SMR_OK;
  if (!num || !den || !out) return SMR_ERR_ARG;
  for (uint32_t i = 0; i < n; i++) if (den[i] == 0) { set_err(c, "smr_rows_fmt_batch: a denominator of 0"); return SMR_ERR_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  DevBuf<uint32_t> d_num, d_den; DevBuf<uint8_t> d_out;
  int rc;
  if ((rc = d_num.alloc(c, n)) || (rc = d_den.alloc(c, n)) || (rc = d_out.alloc(c, (size_t)n * 16))) return rc;
  HIPCHK(c, hipMemcpyAsync(d_num, num, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipMemcpyAsync(d_den, den, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  launch(c, k_rows_fmt, dim3((n + 255u) / 256u), dim3(256), 0, n, (const uint32_t*)d_num, (const uint32_t*)d_den, d_out);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(out, d_out, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SMR_OK;
}
