// smr_engine_fxsplit.hpp -- host side of smr_fastx_split (included by smr_engine.hip; kernels in smr_fxsplit.hpp): the aligned.* / other.*
// FASTX streams of the selected batch (and, for mates in a file of their own, of a second batch), sized, routed and serialised on the device
// from the text that SMR_FASTX_KEEP left there.  Nine totals cross the bus before the output is sized, then the bytes cross it once: what
// smr_results_fetch + smr_reads_record_text + smr_report_add / _add_pair do on the host one read at a time.

namespace {
FxsSrc fxs_src(const Batch& B) {
  FxsSrc s;
  s.text = B.fx_text; s.n = B.fx_n; s.hoff = B.fx_hoff; s.soff = B.fx_soff; s.len = B.d_len; s.state = B.d_saved;
  return s;
}
}  // namespace

namespace {
// smr_fastx_split (zip = false: `bytes` takes the streams, `off` their offsets) and smr_fastx_split_gz (zip = true: the streams stay on the
// device and go through gz_run, `bytes` takes the gzip members, gz_off their offsets, `off` what the plain call would have returned)
int fxs_split_impl(smr_ctx* c, const char* who, bool zip, int mates, const smr_fxsplit_opts* o, const uint8_t* hit, uint8_t* bytes, uint64_t cap, uint64_t off[9],
                   uint64_t gz_off[9], uint64_t* need) {
  if (!c || !o || !off || (zip && (!gz_off || !need))) return SMR_ERR_ARG;
  const std::string W(who);
  for (int k = 0; k < 9; k++) off[k] = 0;
  if (zip) for (int k = 0; k < 9; k++) gz_off[k] = 0;
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
  for (auto& e : S.ev) if (!e) HIPCHK(c, hipEventCreate(&e));
  for (double& m : S.ms) m = 0.0;
  const uint32_t n = (uint32_t)n64, np = (n + FXS_BLOCK - 1u) / FXS_BLOCK;
  int rc;
  if ((rc = S.rec.reserve(c, n)) || (rc = S.woff.reserve(c, n)) || (rc = S.part.reserve(c, (size_t)np * 8u)) || (rc = S.tot.reserve(c, 9))) return rc;
  if (hit) {
    if ((rc = S.hit.reserve(c, n))) return rc;
    HIPCHK(c, hipMemcpyAsync(S.hit, hit, n, hipMemcpyHostToDevice, c->stream));
  }
  FxsOpts D;
  D.layout = (uint32_t)o->layout; D.fastq = A.fx_fastq; D.paired_in = o->paired_in != 0; D.paired_out = o->paired_out != 0; D.out2 = o->out2 != 0; D.sout = o->sout != 0;
  D.want_aligned = o->want_aligned != 0; D.want_other = o->want_other != 0;
  const FxsSrc a = fxs_src(A), b = fxs_src(M ? *M : A);
  HIPCHK(c, hipEventRecord(S.ev[0], c->stream));
  launch(c, k_fxs_measure, dim3(np), dim3(FXS_BLOCK), 0, n, D, a, b, hit ? (const uint8_t*)S.hit : (const uint8_t*)nullptr, S.rec, S.woff, S.part);
  HIPCHK(c, hipEventRecord(S.ev[1], c->stream));
  launch(c, k_fxs_scan, dim3(1), dim3(FXS_BLOCK), 0, S.part, np, S.tot);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(S.ev[2], c->stream));
  unsigned long long h_tot[9];
  HIPCHK(c, hipMemcpyAsync(h_tot, S.tot, sizeof h_tot, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (int k = 0; k < 9; k++) off[k] = h_tot[k];
  const uint64_t total = h_tot[8];
  if (need) *need = total;
  float f = 0;
  if (hipEventElapsedTime(&f, S.ev[0], S.ev[1]) == hipSuccess) S.ms[0] = f;
  if (hipEventElapsedTime(&f, S.ev[1], S.ev[2]) == hipSuccess) S.ms[1] = f;
  if (zip) {                                           // the streams are written where the plain call stages them, and compressed from there
    *need = 0;
    if (total == 0) return SMR_OK;
    if (S.out.cap() < total + 4u && (rc = S.out.alloc(c, (size_t)((total + (total >> 3) + 4095u) & ~4095ull)))) return rc;
    const uint32_t quads = (n + 3u) / 4u, blocks = std::max(1u, std::min<uint32_t>((quads + 3u) / 4u, (uint32_t)c->n_cu * 16u));
    launch(c, k_fxs_copy, dim3(blocks), dim3(256), 0, n, D, a, b, (const uint4*)S.rec, (const unsigned long long*)S.woff, (const unsigned long long*)S.part,
           (const unsigned long long*)S.tot, S.out);
    HIPCHK(c, hipGetLastError());
    return gz_run(c, who, S.out, off, 8, bytes, cap, gz_off, need);
  }
  if (!bytes) return SMR_OK;
  if (cap < total) { set_err(c, W + ": the streams take " + std::to_string(total) + " bytes, the buffer has " + std::to_string(cap)); return SMR_ERR_CAPACITY; }
  if (total == 0) return SMR_OK;
  if (S.out.cap() < total + 4u && (rc = S.out.alloc(c, (size_t)((total + (total >> 3) + 4095u) & ~4095ull)))) return rc;      // (the next, slightly larger call fits as well)
  const uint32_t quads = (n + 3u) / 4u, blocks = std::max(1u, std::min<uint32_t>((quads + 3u) / 4u, (uint32_t)c->n_cu * 16u));
  HIPCHK(c, hipEventRecord(S.ev[3], c->stream));
  launch(c, k_fxs_copy, dim3(blocks), dim3(256), 0, n, D, a, b, (const uint4*)S.rec, (const unsigned long long*)S.woff, (const unsigned long long*)S.part,
                     (const unsigned long long*)S.tot, S.out);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(S.ev[4], c->stream));
  HIPCHK(c, hipMemcpyAsync(bytes, S.out, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(S.ev[5], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (hipEventElapsedTime(&f, S.ev[3], S.ev[4]) == hipSuccess) S.ms[2] = f;
  if (hipEventElapsedTime(&f, S.ev[4], S.ev[5]) == hipSuccess) S.ms[3] = f;
  return SMR_OK;
}
}  // namespace
extern "C" int smr_fastx_split(smr_ctx* c, int mates, const smr_fxsplit_opts* o, const uint8_t* hit, uint8_t* bytes, uint64_t cap, uint64_t off[9], uint64_t* need) {
  return fxs_split_impl(c, "smr_fastx_split", false, mates, o, hit, bytes, cap, off, nullptr, need);
}
extern "C" int smr_fastx_split_gz(smr_ctx* c, int mates, const smr_fxsplit_opts* o, const uint8_t* hit, uint8_t* gz, uint64_t cap, uint64_t gz_off[9], uint64_t plain_off[9],
                                  uint64_t* need) {
  return fxs_split_impl(c, "smr_fastx_split_gz", true, mates, o, hit, gz, cap, plain_off, gz_off, need);
}
extern "C" int smr_fastx_split_times(const smr_ctx* c, double ms[4]) {
  if (!c || !ms) return SMR_ERR_ARG;
  for (int k = 0; k < 4; k++) ms[k] = c->fxs.ms[k];
  return SMR_OK;
}
