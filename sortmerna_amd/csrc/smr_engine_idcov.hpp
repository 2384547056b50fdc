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
  if (c->tasks_cap < ntot) { if ((rc = dev_alloc(c, &c->d_tasks, 2 * ntot))) return rc; c->tasks_cap = ntot; }     // two lists: few / many operations
  if (!d_out && B.cap_idcov < (size_t)B.n) {
    if ((rc = dev_alloc(c, &B.d_idcov, (size_t)B.n * 4))) return rc;
    B.cap_idcov = B.n;
    HIPCHK(c, hipMemsetAsync(B.d_idcov, 0, (size_t)B.n * 16, c->stream));
  }
  HIPCHK(c, hipMemsetAsync(&B.d_ctr[C_IDCOV_FEW], 0, 24, c->stream));              // C_IDCOV_FEW, C_IDCOV_MANY, C_IDCOV_NOCIG
  uint32_t* few = c->d_tasks; uint32_t* many = c->d_tasks + ntot;
  hipLaunchKernelGGL(k_idcov_collect, dim3((uint32_t)((ntot + 1023) / 1024)), dim3(1024), 0, c->stream, B.n, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln,
                     index_num, part, few, many, B.d_ctr, (int)C_IDCOV_FEW);
  HIPCHK(c, hipGetLastError());
  std::vector<unsigned long long> h;
  if ((rc = read_ctr(c, h))) return rc;
  if (h[C_IDCOV_NOCIG]) {
    set_err(c, "smr_idcov_part: " + std::to_string(h[C_IDCOV_NOCIG]) + " alignments of this (index, part) have no CIGAR yet (call smr_traceback first)");
    return SMR_ERR_STATE;
  }
  const uint32_t n_few = (uint32_t)h[C_IDCOV_FEW], n_many = (uint32_t)h[C_IDCOV_MANY];
  if (n_few + n_many == 0) return SMR_OK;
  B.fetched = false;
  if (!d_out) B.idcov_ran = true;
  uint32_t* per_read = d_out ? nullptr : B.d_idcov;
  ev_mark(c, KP_IDCOV);
  if (n_few) hipLaunchKernelGGL(k_idcov_few, dim3(std::min<uint32_t>((n_few + 3u) / 4u, (uint32_t)c->n_cu * 16u)), dim3(64), 0, c->stream, dreads(c), dindex(di), (const uint32_t*)few, n_few,
                                B.d_saved_aln, (const uint32_t*)B.d_cigar, B.slots, min_id, min_cov, per_read, d_out, B.d_ctr, (int)C_IDCOV);
  if (n_many) hipLaunchKernelGGL(k_idcov_many, dim3(std::min<uint32_t>(n_many, (uint32_t)c->n_cu * 16u)), dim3(64), 0, c->stream, dreads(c), dindex(di), (const uint32_t*)many, n_many,
                                 B.d_saved_aln, (const uint32_t*)B.d_cigar, B.slots, min_id, min_cov, per_read, d_out, B.d_ctr, (int)C_IDCOV);
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
  Batch* keep = c->b;
  Batch tmp;
  DevIndex di;
  std::vector<uint32_t> words, lens(n);
  std::vector<uint64_t> rec_off((size_t)n + 1, 0);
  std::vector<RState> st(n);
  std::vector<AlignRec> al(n);
  uint32_t max_len = 1;
  if (cigar_off[n] >= 0xFFFFFFF0ull) { set_err(c, "smr_idcov_batch: too many CIGAR operations"); return SMR_ERR_ARG; }
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
    const uint32_t cw = (uint32_t)((m + 15) >> 4), mw = (uint32_t)((m + 31) >> 5);
    rec_off[i] = words.size();
    words.resize(words.size() + cw + mw, 0u);
    uint32_t* rec = words.data() + rec_off[i];
    for (uint64_t q = 0; q < m; q++) {
      const uint8_t ch = reads[read_off[i] + q];
      if (ch > 3) rec[cw + (q >> 5)] |= 1u << (q & 31); else rec[q >> 4] |= (uint32_t)ch << ((q & 15) * 2);
    }
    lens[i] = (uint32_t)m; max_len = std::max(max_len, (uint32_t)m);
    memset(&st[i], 0, sizeof(RState)); st[i].n_align = 1; st[i].is_hit = 1;
    memset(&al[i], 0, sizeof(AlignRec));
    al[i].ref_num = i; al[i].ref_begin1 = 0; al[i].ref_end1 = (int32_t)qb - 1; al[i].read_begin1 = read_begin[i]; al[i].read_end1 = read_end[i];
    al[i].readlen = readlen[i]; al[i].strand = 1; al[i].has_cigar = 1; al[i].cigar_off = (uint32_t)cigar_off[i]; al[i].cigar_len = (uint32_t)nc;
  }
  rec_off[n] = words.size();
  tmp.n = n; tmp.max_len = max_len; tmp.slots = 1; tmp.used = true;
  uint32_t* d_out = nullptr;
  auto run = [&]() -> int {
    int r2;
    c->b = &tmp;
    if ((r2 = dev_alloc(c, &tmp.d_words, words.size() + 4))) return r2;
    if ((r2 = dev_alloc(c, &tmp.d_rec_off, rec_off.size()))) return r2;
    if ((r2 = dev_alloc(c, &tmp.d_len, lens.size()))) return r2;
    if ((r2 = dev_alloc(c, &tmp.d_saved, (size_t)n))) return r2;
    if ((r2 = dev_alloc(c, &tmp.d_saved_aln, (size_t)n))) return r2;
    if ((r2 = dev_alloc(c, &tmp.d_ctr, (size_t)C_TOTAL))) return r2;
    if ((r2 = dev_alloc(c, &tmp.d_cigar, (size_t)cigar_off[n] + 1))) return r2;
    if ((r2 = dev_alloc(c, &di.ref_seq, (size_t)ref_off[n] + 64))) return r2;
    if ((r2 = dev_alloc(c, &di.ref_off, (size_t)n + 1))) return r2;
    if ((r2 = dev_alloc(c, &d_out, (size_t)n * 4))) return r2;
    HIPCHK(c, hipMemsetAsync(tmp.d_words + words.size(), 0, 16, c->stream));
    HIPCHK(c, hipMemcpyAsync(tmp.d_words, words.data(), words.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tmp.d_rec_off, rec_off.data(), rec_off.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tmp.d_len, lens.data(), lens.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tmp.d_saved, st.data(), st.size() * sizeof(RState), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(tmp.d_saved_aln, al.data(), al.size() * sizeof(AlignRec), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(tmp.d_ctr, 0, C_TOTAL * 8, c->stream));
    HIPCHK(c, hipMemcpyAsync(tmp.d_cigar, cigars, (size_t)cigar_off[n] * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(di.ref_seq + ref_off[n], 0, 64, c->stream));
    if (ref_off[n]) HIPCHK(c, hipMemcpyAsync(di.ref_seq, refs, (size_t)ref_off[n], hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(di.ref_off, ref_off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    di.n_refs = n; di.lnwin = 18; di.used = true;
    if ((r2 = idcov_core(c, di, 0, 0, min_id, min_cov, d_out))) return r2;
    HIPCHK(c, hipMemcpyAsync(out, d_out, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SMR_OK;
  };
  const int rc = run();
  (void)hipStreamSynchronize(c->stream);
  c->b = keep;
  dev_free(&tmp.d_words); dev_free(&tmp.d_rec_off); dev_free(&tmp.d_len); dev_free(&tmp.d_saved); dev_free(&tmp.d_saved_aln); dev_free(&tmp.d_ctr); dev_free(&tmp.d_cigar);
  dev_free(&di.ref_seq); dev_free(&di.ref_off); dev_free(&d_out);
  return rc;
}
