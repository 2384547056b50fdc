// smr_engine_fastx.hpp -- host side of smr_reads_upload_fastx* (included by smr_engine.hip; kernels in smr_fastx.hpp): the text goes to the
// device, the kernels find lines and records and say whether the text is regular, one small D2H brings the totals the batch is reserved
// from, k_fx_pack writes the batch.  Irregular or malformed text -- and empty text -- is the host parser's (smr::load_fastx_bytes): the answer
// or the refusal is then the host's by construction.  Nothing of the batch is touched before the text is known to be good.

namespace {
void fx_report(smr_ctx* c, uint64_t path, uint64_t lines, uint64_t records, uint64_t bytes, const double* ms) {
  std::lock_guard<std::mutex> l_(c->err_m);
  c->fx_info[0] = path; c->fx_info[1] = lines; c->fx_info[2] = records; c->fx_info[3] = bytes;
  for (int k = 0; k < 5; k++) c->fx_ms[k] = ms ? ms[k] : 0.0;
}
// a smr_reads without its packed words (SMR_FASTX_VIEW)
void fx_make_view(smr_reads* r) {
  std::vector<uint32_t>().swap(r->words); std::vector<uint64_t>().swap(r->rec_off);
  r->view = true;
}
// SMR_FASTX_KEEP on the host parser's path: the text, padded like fastx_upload pads it, and the parser's record offsets go to the batch
int fx_keep_host(smr_ctx* c, Batch& B, hipStream_t st, const char* text, size_t n, const smr_reads* r) {
  const size_t cap = ((n + 15u) & ~(size_t)15u) + 64u;
  int rc;
  if ((rc = B.fx_text.alloc(c, cap)) || (rc = B.fx_hoff.alloc(c, r->n)) || (rc = B.fx_soff.alloc(c, r->n))) return rc;
  if (n) HIPCHK(c, hipMemcpyAsync(B.fx_text, text, n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(B.fx_text + n, '\n', cap - n, st));
  if (r->n) {
    HIPCHK(c, hipMemcpyAsync(B.fx_hoff, r->hdr_off.data(), (size_t)r->n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(B.fx_soff, r->seq_off.data(), (size_t)r->n * 8, hipMemcpyHostToDevice, st));
  }
  HIPCHK(c, hipStreamSynchronize(st));
  B.fx_n = (uint32_t)n; B.fx_fastq = r->fastq; B.fx_kept = true;
  return SMR_OK;
}
int fx_host_path(smr_ctx* c, Batch& B, hipStream_t st, const char* name, const char* text, size_t n, const std::shared_ptr<void>& owner, uint32_t max_aln, uint32_t flags,
                 smr_reads** out, uint64_t lines, uint64_t bytes) {
  smr_reads* r = nullptr; std::string why;
  int rc = smr::load_fastx_bytes(name, text, n, owner, 0, true, &r, why);
  if (rc != SMR_OK) { set_err(c, why); return rc; }
  rc = upload_into(c, B, r, max_aln, st);
  if (rc == SMR_OK && (flags & SMR_FASTX_KEEP)) rc = fx_keep_host(c, B, st, text, n, r);
  if (rc != SMR_OK) { delete r; return rc; }
  fx_report(c, 1, lines, r->n, bytes, nullptr);
  if (out) { if (flags & SMR_FASTX_VIEW) fx_make_view(r); *out = r; } else delete r;
  return SMR_OK;
}

#define FX_TEXT_LIMIT (0xFFFFFFFFull - 63ull)      // 2^32 - 64: text of that many bytes or more is SMR_ERR_CAPACITY
// SMR_FASTX_INFLATE: the gzip file at gz -> its text, in S.text on the device (on_device; text_n bytes, the host has none of them yet), or,
// where the device does not settle the file, inflated by zlib into a buffer `owner` keeps (the host's answer, or its refusal under `name`)
int fx_inflate(smr_ctx* c, FxScratch& S, GunzScratch& G, hipStream_t st, const char* name, const uint8_t* gz, uint64_t n, std::shared_ptr<void>& owner, const char*& text,
               uint64_t& text_n, bool& on_device) {
  uint64_t plain = 0;
  int rc = gunz_device(c, G, st, gz, n, 0, S.text, &plain, &on_device, FX_TEXT_LIMIT);
  if (rc) return rc;
  if (on_device) { owner.reset(); text = nullptr; text_n = plain; return SMR_OK; }
  if (plain >= FX_TEXT_LIMIT) { owner.reset(); text = ""; text_n = plain; return SMR_OK; }      // (known after the counting pass: fastx_upload refuses it before it touches the text)
  auto v = std::make_shared<std::vector<char>>();
  std::string why;
  if (!smr::gunzip_bytes(name, gz, (size_t)n, *v, why)) { set_err(c, why); return SMR_ERR_IO; }
  owner = v; text = v->empty() ? "" : v->data(); text_n = v->size();
  return SMR_OK;
}
inline bool fx_is_gzip(const void* p, uint64_t n) { return n >= 2 && ((const uint8_t*)p)[0] == 0x1Fu && ((const uint8_t*)p)[1] == 0x8Bu; }

// on_device: the n64 bytes of text are in S.text already (fx_inflate) and `text` is not given.  The host then reads back what it needs: all of
// the text once for *out or for the host parser, otherwise the first bytes, which say the format.
int fastx_upload(smr_ctx* c, Batch& B, FxScratch& S, hipStream_t st, const char* name, const char* text, uint64_t n64, std::shared_ptr<void> owner, uint32_t max_aln,
                 uint32_t flags, smr_reads** out, bool on_device = false) {
  if (n64 >= FX_TEXT_LIMIT) { set_err(c, "smr_reads_upload_fastx: 2^32 - 64 bytes of text or more: hand the text over in pieces that end at record boundaries"); return SMR_ERR_CAPACITY; }
  if (max_aln == 0) max_aln = 1;
  if (out) *out = nullptr;
  const uint32_t n = (uint32_t)n64;
  int rc;
  uint32_t have = n;                                   // bytes of the text the host can read
  std::vector<char> head;
  auto fetch = [&]() -> int {                           // (on_device) the whole text, once
    if (have == n && text) return SMR_OK;
    auto v = std::make_shared<std::vector<char>>((size_t)n + 1u);
    if (n) HIPCHK(c, hipMemcpyAsync(v->data(), S.text, n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    owner = v; text = v->data(); have = n;
    return SMR_OK;
  };
  if (on_device) {
    if (out) { if ((rc = fetch())) return rc; }
    else {
      have = std::min<uint32_t>(n, 4096u);
      head.resize((size_t)have + 1u);
      if (have) HIPCHK(c, hipMemcpyAsync(head.data(), S.text, have, hipMemcpyDeviceToHost, st));
      HIPCHK(c, hipStreamSynchronize(st));
      text = head.data();
    }
  }
  uint32_t first = 0;
  while (first < have && (text[first] == '\n' || text[first] == '\r')) first++;
  if (first >= have && have < n) {                      // (nothing but line ends so far)
    if ((rc = fetch())) return rc;
    while (first < n && (text[first] == '\n' || text[first] == '\r')) first++;
  }
  // no record at all, or neither format: the host parser's batch of 0 reads / its message
  if (first >= n || (text[first] != '@' && text[first] != '>')) { if ((rc = fetch())) return rc; return fx_host_path(c, B, st, name, text, n, owner, max_aln, flags, out, 0, 0); }
  const uint32_t fastq = text[first] == '@';
  if ((rc = S.clk.begin(c))) return rc;
  // ---- the text, padded for the aligned loads of the kernels
  const size_t cap = (((size_t)n + 15u) & ~(size_t)15u) + 64u;
  const uint32_t nt = (uint32_t)(((uint64_t)n + FX_TILE - 1u) / FX_TILE);
  if ((rc = S.text.reserve(c, cap)) || (rc = S.tot.reserve(c, FXT_COUNT)) || (rc = S.part_t.reserve(c, nt))) return rc;
  uint32_t h_tot[FXT_COUNT] = {};
  h_tot[FXT_FIRST_BLANK_HDR] = ~0u; h_tot[FXT_MIN_LEN] = ~0u;
  if ((rc = S.clk.mark(c, 0, st))) return rc;
  if (!on_device) HIPCHK(c, hipMemcpyAsync(S.text, text, n, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipMemsetAsync(S.text + n, '\n', cap - n, st));
  HIPCHK(c, hipMemcpyAsync(S.tot, h_tot, sizeof h_tot, hipMemcpyHostToDevice, st));
  if ((rc = S.clk.mark(c, 1, st))) return rc;
  // ---- lines
  launch_on(st, k_fx_count, dim3(nt), dim3(FX_BLOCK), 0, (const uint8_t*)S.text, n, first, (uint32_t*)S.part_t);
  launch_on(st, k_fx_scan, dim3(1), dim3(FX_LBLOCK), 0, (uint32_t*)S.part_t, (uint32_t*)nullptr, nt, (uint32_t*)S.tot, (uint32_t)FXT_NEWLINES, 0u);
  HIPCHK(c, hipGetLastError());
  uint32_t newlines = 0;
  HIPCHK(c, hipMemcpyAsync(&newlines, S.tot + FXT_NEWLINES, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  const uint32_t nl = newlines + 1u, nlb = (nl + FX_LBLOCK - 1u) / FX_LBLOCK;
  const size_t per_line = (size_t)nl + 1u;
  const size_t max_rec = fastq ? (size_t)nl / 4u + 2u : per_line;              // (what the record arrays can be asked to hold: R + 1 entries)
  const uint32_t nrb = (uint32_t)((max_rec + FX_LBLOCK - 1u) / FX_LBLOCK), npart = std::max(nlb, nrb);
  if ((rc = S.line_start.reserve(c, per_line)) || (rc = S.lrec.reserve(c, per_line)) || (rc = S.lcum.reserve(c, per_line)) || (rc = S.part_l.reserve(c, (size_t)3 * npart)) ||
      (rc = S.hdr_line.reserve(c, max_rec)) || (rc = S.rcum.reserve(c, max_rec)) || (rc = S.rlen.reserve(c, max_rec)) || (rc = S.rwi.reserve(c, max_rec)) ||
      (rc = S.hoff.reserve(c, max_rec)) || (rc = S.soff.reserve(c, max_rec))) return rc;
  uint32_t* const part_h = S.part_l; uint32_t* const part_c = part_h + npart; uint32_t* const part_w = part_c + npart;
  launch_on(st, k_fx_lines, dim3(nt), dim3(FX_BLOCK), 0, (const uint8_t*)S.text, n, first, (const uint32_t*)S.part_t, (const uint32_t*)S.tot, (uint32_t*)S.line_start);
  if ((rc = S.clk.mark(c, 2, st))) return rc;
  // ---- records
  launch_on(st, k_fx_classify, dim3(nlb), dim3(FX_LBLOCK), 0, (const uint8_t*)S.text, fastq, nl, (const uint32_t*)S.line_start, (uint32_t*)S.lrec, (uint32_t*)S.lcum, part_h, part_c,
                     (uint32_t*)S.tot);
  launch_on(st, k_fx_scan, dim3(1), dim3(FX_LBLOCK), 0, part_h, part_c, nlb, (uint32_t*)S.tot, (uint32_t)FXT_RECORDS, (uint32_t)FXT_TOTAL_LEN);
  launch_on(st, k_fx_records, dim3(nlb), dim3(FX_LBLOCK), 0, fastq, nl, (const uint32_t*)S.lrec, (uint32_t*)S.lcum, (const uint32_t*)part_h, (const uint32_t*)part_c,
                     (uint32_t*)S.hdr_line, (uint32_t*)S.rcum, (uint32_t*)S.tot);
  // (a FASTQ text that turns out irregular can count more headers than max_rec allows for: lines 4k are at most nl / 4 + 1, so it cannot)
  launch_on(st, k_fx_reclen, dim3(nrb), dim3(FX_LBLOCK), 0, n, (const uint32_t*)S.line_start, (const uint32_t*)S.hdr_line, (const uint32_t*)S.rcum, (uint32_t*)S.tot,
                     (uint32_t*)S.rlen, (uint32_t*)S.rwi, part_w, (unsigned long long*)S.hoff, (unsigned long long*)S.soff);
  launch_on(st, k_fx_scan, dim3(1), dim3(FX_LBLOCK), 0, part_w, (uint32_t*)nullptr, nrb, (uint32_t*)S.tot, (uint32_t)FXT_WORDS, 0u);
  HIPCHK(c, hipGetLastError());
  if ((rc = S.clk.mark(c, 3, st))) return rc;
  HIPCHK(c, hipMemcpyAsync(h_tot, S.tot, sizeof h_tot, hipMemcpyDeviceToHost, st));
  HIPCHK(c, hipStreamSynchronize(st));
  if (h_tot[FXT_FLAG]) { if ((rc = fetch())) return rc; return fx_host_path(c, B, st, name, text, n, owner, max_aln, flags, out, nl, n); }
  // ---- the batch
  const uint32_t R = h_tot[FXT_RECORDS], W = h_tot[FXT_WORDS];
  if ((rc = batch_reserve(c, B, W, R, h_tot[FXT_MIN_LEN], h_tot[FXT_MAX_LEN], max_aln, st))) return rc;
  const uint32_t chunks = (R + 63u) / 64u, blocks = std::max(1u, std::min<uint32_t>((chunks + 3u) / 4u, (uint32_t)c->n_cu * 16u));
  launch_on(st, k_fx_pack, dim3(blocks), dim3(256), 0, (const uint8_t*)S.text, R, (const uint32_t*)S.line_start, (const uint32_t*)S.lcum, (const uint32_t*)S.hdr_line,
                     (const uint32_t*)S.rcum, (const uint32_t*)S.rlen, (const uint32_t*)S.rwi, (const uint32_t*)part_w, (uint32_t*)B.d_len, reinterpret_cast<unsigned long long*>(B.d_rec_off.get()),
                     (uint32_t*)B.d_words);
  HIPCHK(c, hipGetLastError());
  if ((rc = S.clk.mark(c, 4, st))) return rc;
  if ((rc = batch_fresh_state(c, B, st))) return rc;
  // ---- what the caller asked to see of it
  smr_reads* r = nullptr;
  if (out) {
    r = new smr_reads();
    r->n = R; r->fastq = fastq != 0; r->total_len = h_tot[FXT_TOTAL_LEN]; r->min_len = R ? h_tot[FXT_MIN_LEN] : 0; r->max_len = h_tot[FXT_MAX_LEN];
    r->text_owner = owner; r->text = text; r->text_n = n;
    smr::reserve_huge(r->len, R); smr::reserve_huge(r->hdr_off, R); smr::reserve_huge(r->seq_off, R);      // (2 MB pages for the first touch, as the host parser asks for)
    r->len.resize(R); r->hdr_off.resize(R); r->seq_off.resize(R);
    hipError_t e = hipSuccess;
    if (R) {
      e = hipMemcpyAsync(r->len.data(), B.d_len, (size_t)R * 4, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipMemcpyAsync(r->hdr_off.data(), S.hoff, (size_t)R * 8, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess) e = hipMemcpyAsync(r->seq_off.data(), S.soff, (size_t)R * 8, hipMemcpyDeviceToHost, st);
    }
    if (flags & SMR_FASTX_VIEW) r->view = true;
    else {
      smr::reserve_huge(r->rec_off, (size_t)R + 1); smr::reserve_huge(r->words, W);
      r->rec_off.resize((size_t)R + 1); r->words.resize(W);
      if (e == hipSuccess) e = hipMemcpyAsync(r->rec_off.data(), B.d_rec_off, ((size_t)R + 1) * 8, hipMemcpyDeviceToHost, st);
      if (e == hipSuccess && W) e = hipMemcpyAsync(r->words.data(), B.d_words, (size_t)W * 4, hipMemcpyDeviceToHost, st);
    }
    if (e != hipSuccess) { delete r; return dev_fail(c, "hipMemcpyAsync", e); }
  }
  if ((rc = S.clk.mark(c, 5, st))) { delete r; return rc; }
  const hipError_t e = hipStreamSynchronize(st);
  if (e != hipSuccess) { delete r; return dev_fail(c, "hipStreamSynchronize", e); }
  double ms[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < 5; k++) (void)S.clk.elapsed(k, k + 1, ms[k]);
  fx_report(c, 0, nl, R, n, ms);
  if (flags & SMR_FASTX_KEEP) {                                 // (handed over, not copied: the stream's scratch allocates again on its next use)
    B.fx_text = std::move(S.text); B.fx_hoff = std::move(S.hoff); B.fx_soff = std::move(S.soff);
    B.fx_n = n; B.fx_fastq = fastq != 0; B.fx_kept = true;
  }
  if (out) *out = r;
  return SMR_OK;
}
}  // namespace

extern "C" int smr_reads_upload_fastx(smr_ctx* c, const char* text, uint64_t n_bytes, uint32_t max_aln, uint32_t flags, smr_reads** out) {
  if (!c || !text) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  if ((flags & SMR_FASTX_INFLATE) && fx_is_gzip(text, n_bytes)) {
    std::shared_ptr<void> owner; const char* p = nullptr; uint64_t n = 0; bool on_device = false;
    const int rc = fx_inflate(c, c->fx[0], c->gunz[0], c->stream, "smr_reads_upload_fastx", (const uint8_t*)text, n_bytes, owner, p, n, on_device);
    return rc ? rc : fastx_upload(c, *c->b, c->fx[0], c->stream, "", p, n, owner, max_aln, flags, out, on_device);
  }
  return fastx_upload(c, *c->b, c->fx[0], c->stream, "", text, n_bytes, std::shared_ptr<void>(), max_aln, flags, out);
}
extern "C" int smr_reads_upload_fastx_batch(smr_ctx* c, int batch, const char* text, uint64_t n_bytes, uint32_t max_aln, uint32_t flags, smr_reads** out) {
  if (!c || !text || batch < 0 || batch >= SMR_MAX_BATCHES) return SMR_ERR_ARG;
  {
    std::lock_guard<std::mutex> l(c->sel_m);
    if (&c->bt[batch] == c->b) { std::lock_guard<std::mutex> l2(c->err_m); c->err = "smr_reads_upload_fastx_batch: the batch is the selected one (use smr_reads_upload_fastx)"; return SMR_ERR_STATE; }
  }
  HIPCHK(c, hipSetDevice(c->device));
  if ((flags & SMR_FASTX_INFLATE) && fx_is_gzip(text, n_bytes)) {
    std::shared_ptr<void> owner; const char* p = nullptr; uint64_t n = 0; bool on_device = false;
    const int rc = fx_inflate(c, c->fx[1], c->gunz[1], c->upload_stream, "smr_reads_upload_fastx_batch", (const uint8_t*)text, n_bytes, owner, p, n, on_device);
    return rc ? rc : fastx_upload(c, c->bt[batch], c->fx[1], c->upload_stream, "", p, n, owner, max_aln, flags, out, on_device);
  }
  return fastx_upload(c, c->bt[batch], c->fx[1], c->upload_stream, "", text, n_bytes, std::shared_ptr<void>(), max_aln, flags, out);
}
extern "C" int smr_reads_upload_fastx_file(smr_ctx* c, const char* path, uint32_t max_aln, uint32_t flags, smr_reads** out, char* err, size_t errcap) {
  if (!c || !path) return SMR_ERR_ARG;
  std::shared_ptr<void> owner; const char* p = nullptr; size_t n = 0; std::string why;
  int rc;
  const bool inflate = (flags & SMR_FASTX_INFLATE) != 0;          // (a gzip file then stays as it is in the mapping)
  if (!smr::fastx_slurp(path, owner, p, n, why, inflate)) { set_err(c, why); rc = SMR_ERR_IO; }
  else if (hipSetDevice(c->device) != hipSuccess) { set_err(c, "hipSetDevice failed"); rc = SMR_ERR_DEVICE; }
  else if (inflate && fx_is_gzip(p, n)) {
    std::shared_ptr<void> towner; const char* t = nullptr; uint64_t tn = 0; bool on_device = false;
    rc = fx_inflate(c, c->fx[0], c->gunz[0], c->stream, path, (const uint8_t*)p, n, towner, t, tn, on_device);
    if (rc == SMR_OK) rc = fastx_upload(c, *c->b, c->fx[0], c->stream, path, t, tn, towner, max_aln, flags, out, on_device);
  }
  else rc = fastx_upload(c, *c->b, c->fx[0], c->stream, path, p ? p : "", n, owner, max_aln, flags, out);
  if (rc != SMR_OK && err && errcap) snprintf(err, errcap, "%s", smr_last_error(c));
  return rc;
}
extern "C" int smr_fastx_info(const smr_ctx* c, uint64_t info[4]) {
  if (!c || !info) return SMR_ERR_ARG;
  std::lock_guard<std::mutex> l_(const_cast<smr_ctx*>(c)->err_m);
  for (int k = 0; k < 4; k++) info[k] = c->fx_info[k];
  return SMR_OK;
}
extern "C" int smr_fastx_times(const smr_ctx* c, double ms[5]) {
  if (!c || !ms) return SMR_ERR_ARG;
  std::lock_guard<std::mutex> l_(const_cast<smr_ctx*>(c)->err_m);
  for (int k = 0; k < 5; k++) ms[k] = c->fx_ms[k];
  return SMR_OK;
}
