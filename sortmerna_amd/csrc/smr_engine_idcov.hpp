// smr_engine_idcov.hpp -- host side of the %id / %coverage pass (included by smr_engine.hip; kernels in smr_idcov.hpp): smr_idcov_part,
// smr_idcov_counters, smr_idcov_counters_device, smr_idcov_batch.

// The pass over the stored alignments of (index_num, part) of the selected batch, whose reference sequences are di's.  d_out: the seam's
// {n_miss, n_gap, n_match, class} per alignment slot instead of the per-read counters.
static int idcov_core(smr_ctx* c, const DevIndex& di, uint32_t index_num, uint32_t part, double min_id, double min_cov, uint32_t* d_out) {
  int rc;
  Batch& B = *c->b;
  ev_drop(c);
  const uint64_t ntot = (uint64_t)B.n * B.slots;
  if (ntot >= 0xFFFFFC00ull) { set_err(c, "smr_idcov_part: reads x alignment slots of the batch must stay below 2^32 (the work lists index them with 32 bits)"); return SMR_ERR_CAPACITY; }
  if ((rc = c->d_tasks.reserve(c, 2 * ntot))) return rc;     // two lists: few / many operations
  if (!d_out && B.d_idcov.cap() < (size_t)B.n * 4) {
    if ((rc = B.d_idcov.alloc(c, (size_t)B.n * 4))) return rc;
    HIPCHK(c, hipMemsetAsync(B.d_idcov, 0, (size_t)B.n * 16, c->stream));
  }
  HIPCHK(c, hipMemsetAsync(&B.d_ctr[C_IDCOV_FEW], 0, 24, c->stream));              // C_IDCOV_FEW, C_IDCOV_MANY, C_IDCOV_NOCIG
  uint32_t* few = c->d_tasks; uint32_t* many = c->d_tasks + ntot;
  launch(c, k_idcov_collect, dim3((uint32_t)((ntot + 1023) / 1024)), dim3(1024), 0, B.n, B.slots, B.d_saved, B.d_saved_aln, index_num, part, few, many, B.d_ctr, (int)C_IDCOV_FEW);
  HIPCHK(c, hipGetLastError());
  std::vector<unsigned long long> h;
  if ((rc = read_ctr(c, h))) return rc;
  if ((rc = part_refuse_state(c, "smr_idcov_part", (uint32_t)h[C_IDCOV_NOCIG], 0, 0))) return rc;      // (a count of slots: below ntot)
  const uint32_t n_few = (uint32_t)h[C_IDCOV_FEW], n_many = (uint32_t)h[C_IDCOV_MANY];
  if (n_few + n_many == 0) return SMR_OK;
  B.fetched = false;
  if (!d_out) B.idcov_ran = true;
  uint32_t* per_read = d_out ? nullptr : B.d_idcov.get();
  ev_mark(c, KP_IDCOV);
  if (n_few) launch(c, k_idcov_few, dim3(std::min<uint32_t>((n_few + 3u) / 4u, (uint32_t)c->n_cu * 16u)), dim3(64), 0, dreads(c), dindex(di), few, n_few,
                    B.d_saved_aln, B.d_cigar, B.slots, min_id, min_cov, per_read, d_out, B.d_ctr, (int)C_IDCOV);
  if (n_many) launch(c, k_idcov_many, dim3(std::min<uint32_t>(n_many, (uint32_t)c->n_cu * 16u)), dim3(64), 0, dreads(c), dindex(di), many, n_many,
                     B.d_saved_aln, B.d_cigar, B.slots, min_id, min_cov, per_read, d_out, B.d_ctr, (int)C_IDCOV);
  ev_stop(c);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipStreamSynchronize(c->stream));
  ev_collect(c);
  return SMR_OK;
}

static bool idcov_threshold_ok(double x) { return x >= 0.0 && x <= 1.0; }       // (false for a NaN)

// denovo_stats for ONE (index, part) over the selected batch (processor.cpp:287-366): every stored alignment of that part is classified once
// -- a second call finds them marked and changes nothing.  The reference runs this pass after ALL alignment is done; an alignment that a later
// smr_align_part replaced would have been counted for nothing, so smr_align_part refuses a batch of which the pass has counted an alignment
// (smr_state_reset or an upload starts over; a call that found nothing to count leaves the batch as it was).
extern "C" int smr_idcov_part(smr_ctx* c, int slot, const smr_params* p, double min_id, double min_cov) {
  if (!c || slot < 0 || slot >= 64) return SMR_ERR_ARG;
  if (!c->idx[slot].used || !c->b->d_saved) { set_err(c, "index slot empty or no reads uploaded"); return SMR_ERR_STATE; }
  if (!idcov_threshold_ok(min_id) || !idcov_threshold_ok(min_cov)) { set_err(c, "smr_idcov_part: min_id and min_cov must be within [0, 1]"); return SMR_ERR_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  int rc = check_params(c, p, false); if (rc) return rc;
  if (c->b->n == 0) return SMR_OK;
  return idcov_core(c, c->idx[slot], p->index_num, p->part, min_id, min_cov, nullptr);
}

// Readstats::n_yid_ycov, n_yid_ncov, n_nid_ycov, num_denovo of the selected batch (readstats.hpp:77-85)
extern "C" int smr_idcov_counters(smr_ctx* c, uint64_t out[4]) {
  if (!c || !out) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  std::vector<unsigned long long> h;
  int rc = read_ctr(c, h); if (rc) return rc;
  for (int k = 0; k < 4; k++) out[k] = h[C_IDCOV + k];
  return SMR_OK;
}
extern "C" int smr_idcov_counters_device(smr_ctx* c, void** dptr, uint32_t* n_u64) {
  if (!c || !dptr || !n_u64) return SMR_ERR_ARG;
  if (!c->b->d_ctr) { set_err(c, "smr_idcov_counters_device: the selected batch has no counter block yet"); return SMR_ERR_STATE; }
  *dptr = c->b->d_ctr + C_IDCOV; *n_u64 = 4;
  return SMR_OK;
}

// The kernels at the seam of Read::calc_miss_gap_match + the decision of denovo_stats_run: a throw-away batch / reference set is put on the
// device, one stored alignment per triple, and goes through the same collect / k_idcov_few / k_idcov_many as smr_idcov_part.
extern "C" int smr_idcov_batch(smr_ctx* c, uint32_t n, const uint8_t* reads, const uint64_t* read_off, const uint8_t* refs, const uint64_t* ref_off,
                               const uint32_t* cigars, const uint64_t* cigar_off, const int32_t* read_begin, const int32_t* read_end, const uint32_t* readlen,
                               double min_id, double min_cov, uint32_t* out) {
  if (!c || !read_off || !ref_off || !cigar_off || !read_begin || !read_end || !readlen || !out) return SMR_ERR_ARG;
  if (!idcov_threshold_ok(min_id) || !idcov_threshold_ok(min_cov)) { set_err(c, "smr_idcov_batch: min_id and min_cov must be within [0, 1]"); return SMR_ERR_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  if (n == 0) return SMR_OK;
  if (!reads || !refs || !cigars) return SMR_ERR_ARG;
  if (cigar_off[n] >= 0xFFFFFFF0ull) { set_err(c, "smr_idcov_batch: too many CIGAR operations"); return SMR_ERR_ARG; }
  std::vector<uint64_t> ref_span(n);                       // reference letters each CIGAR covers
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t m = read_off[i + 1] - read_off[i], nr = ref_off[i + 1] - ref_off[i], nc = cigar_off[i + 1] - cigar_off[i];
    if (m == 0 || m > 0xFFFFu || nc == 0 || readlen[i] == 0 || read_begin[i] < 0 || (uint64_t)read_begin[i] >= m) { set_err(c, "smr_idcov_batch: empty or oversized triple"); return SMR_ERR_ARG; }
    // the CIGAR must stay inside the read and the reference window (the kernels would count what lies outside as mismatches; a caller's mistake is said here)
    uint64_t pb = (uint64_t)read_begin[i], qb = 0;
    for (uint64_t q = 0; q < nc; q++) {
      const uint32_t cg = cigars[cigar_off[i] + q], op = cg & 0xFu, len = cg >> 4;
      if (op > 2) { set_err(c, "smr_idcov_batch: CIGAR operations are 0 / 1 / 2 (M / I / D)"); return SMR_ERR_ARG; }
      if (op != 2) pb += len;
      if (op != 1) qb += len;
    }
    if (pb > m || qb > nr) { set_err(c, "smr_idcov_batch: a CIGAR runs past its read or its reference window"); return SMR_ERR_ARG; }
    ref_span[i] = qb;
  }
  TempBatch t(c);
  t.pack(n, reads, read_off);
  for (uint32_t i = 0; i < n; i++) {                        // one stored alignment per triple, with the caller's CIGAR
    AlignRec& a = t.al[i];
    a.ref_begin1 = 0; a.ref_end1 = (int32_t)ref_span[i] - 1; a.read_begin1 = read_begin[i]; a.read_end1 = read_end[i];
    a.readlen = readlen[i]; a.has_cigar = 1; a.cigar_off = (uint32_t)cigar_off[i]; a.cigar_len = (uint32_t)(cigar_off[i + 1] - cigar_off[i]);
  }
  DevBuf<uint32_t> d_out;
  int rc;
  if ((rc = t.upload(refs, ref_off)) || (rc = t.b.d_cigar.alloc(c, (size_t)cigar_off[n] + 1)) || (rc = d_out.alloc(c, (size_t)n * 4))) return rc;
  HIPCHK(c, hipMemcpyAsync(t.b.d_cigar, cigars, (size_t)cigar_off[n] * 4, hipMemcpyHostToDevice, c->stream));
  if ((rc = idcov_core(c, t.di, 0, 0, min_id, min_cov, d_out))) return rc;
  HIPCHK(c, hipMemcpyAsync(out, d_out, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SMR_OK;
}
