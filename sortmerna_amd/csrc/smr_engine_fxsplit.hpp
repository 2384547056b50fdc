// smr_engine_fxsplit.hpp -- host side of smr_fastx_split*, smr_fastx_denovo* (included by smr_engine.hip behind smr_engine_gzip.hpp; kernels in
// smr_fxsplit.hpp): the aligned.* / other.* and the aligned_denovo.* FASTX streams of the selected batch (and, for mates in a file of their
// own, of a second batch), sized, routed and serialised on the device from the text that SMR_FASTX_KEEP left there.  Nine totals cross the bus
// before the output is sized, then the bytes cross it once -- or stay and are compressed there (gz_run): what smr_results_fetch +
// smr_reads_record_text + smr_report_add / _add_pair do on the host one read at a time.

namespace {
FxsSrc fxs_src(const Batch& B) {
  FxsSrc s;
  s.text = B.fx_text; s.n = B.fx_n; s.hoff = B.fx_hoff; s.soff = B.fx_soff; s.len = B.d_len; s.state = B.d_saved;
  return s;
}
// The writer behind smr_fastx_split* (denovo = false: eight streams routed by is_hit or `flags`, k_fxs_measure; the call of smr_fastx_split_times)
// and smr_fastx_denovo* (denovo = true: the four aligned_denovo.* streams of the reads the %id / %coverage pass counted as de novo, or of
// `flags`, k_fxs_dn_measure; keeps no times).  zip = false: `bytes` takes the streams, `off` their offsets; zip = true: the streams stay on the
// device and go through gz_run, `bytes` takes the gzip members, gz_off their offsets, `off` what the plain call would have returned
int fxs_impl(smr_ctx* c, const char* who, bool denovo, bool zip, int mates, const smr_fxsplit_opts* o, const uint8_t* flags, uint8_t* bytes, uint64_t cap, uint64_t* off,
             uint64_t* gz_off, uint64_t* need) {
  if (!c || !o || !off || (zip && (!gz_off || !need))) return SMR_ERR_ARG;
  const std::string W(who);
  const uint32_t ns = denovo ? 4u : 8u;
  for (uint32_t k = 0; k <= ns; k++) off[k] = 0;
  if (zip) for (uint32_t k = 0; k <= ns; k++) gz_off[k] = 0;
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
  int rc;
  if (!denovo && (rc = S.clk.begin(c))) return rc;
  auto mark = [&](int i) { return denovo ? SMR_OK : S.clk.mark(c, i, c->stream); };
  const uint32_t n = (uint32_t)n64, np = (n + FXS_BLOCK - 1u) / FXS_BLOCK;
  if ((rc = S.rec.reserve(c, n)) || (rc = S.woff.reserve(c, n)) || (rc = S.part.reserve(c, (size_t)np * 8u)) || (rc = S.tot.reserve(c, 9))) return rc;
  if (flags) {
    if ((rc = S.hit.reserve(c, n))) return rc;
    HIPCHK(c, hipMemcpyAsync(S.hit, flags, n, hipMemcpyHostToDevice, c->stream));
  }
  const uint8_t* d_flags = flags ? (const uint8_t*)S.hit : (const uint8_t*)nullptr;
  FxsOpts D;
  D.layout = (uint32_t)o->layout; D.fastq = A.fx_fastq; D.paired_in = o->paired_in != 0; D.paired_out = o->paired_out != 0; D.out2 = o->out2 != 0; D.sout = o->sout != 0;
  D.want_aligned = denovo || o->want_aligned != 0; D.want_other = !denovo && o->want_other != 0;
  const FxsSrc a = fxs_src(A), b = fxs_src(M ? *M : A);
  if ((rc = mark(0))) return rc;
  if (denovo) {
    // the counters of a batch on which the pass never ran hold nothing: no de novo read
    auto counters = [](const Batch& X) { return X.d_idcov && X.d_idcov.cap() >= (size_t)X.n * 4 ? (const uint32_t*)X.d_idcov : (const uint32_t*)nullptr; };
    launch(c, k_fxs_dn_measure, dim3(np), dim3(FXS_BLOCK), 0, n, D, a, b, counters(A), counters(M ? *M : A), d_flags, S.rec, S.woff, S.part);
  } else launch(c, k_fxs_measure, dim3(np), dim3(FXS_BLOCK), 0, n, D, a, b, d_flags, S.rec, S.woff, S.part);
  if ((rc = mark(1))) return rc;
  launch(c, k_fxs_scan, dim3(1), dim3(FXS_BLOCK), 0, S.part, np, S.tot);
  HIPCHK(c, hipGetLastError());
  if ((rc = mark(2))) return rc;
  unsigned long long h_tot[9];
  HIPCHK(c, hipMemcpyAsync(h_tot, S.tot, sizeof h_tot, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (uint32_t k = 0; k <= ns; k++) off[k] = h_tot[k];
  const uint64_t total = h_tot[ns];                    // (de novo: streams 4..7 stay empty, tot[4..8] all hold the end of stream 3)
  if (need) *need = total;
  if (!denovo) { S.clk.set(0, 0, 1); S.clk.set(1, 1, 2); }
  if (zip) *need = 0;                                  // (until gz_run knows the size of the members)
  else {
    if (!bytes) return SMR_OK;
    if (cap < total) { set_err(c, W + ": the streams take " + std::to_string(total) + " bytes, the buffer has " + std::to_string(cap)); return SMR_ERR_CAPACITY; }
  }
  if (total == 0) return SMR_OK;
  // the streams, staged on the device: copied to the host from there, or compressed from there
  if ((rc = S.out.reserve_headroom(c, (size_t)total, 4))) return rc;
  const uint32_t quads = (n + 3u) / 4u, blocks = std::max(1u, std::min<uint32_t>((quads + 3u) / 4u, (uint32_t)c->n_cu * 16u));
  if (!zip && (rc = mark(3))) return rc;
  launch(c, k_fxs_copy, dim3(blocks), dim3(256), 0, n, D, a, b, (const uint4*)S.rec, (const unsigned long long*)S.woff, (const unsigned long long*)S.part,
         (const unsigned long long*)S.tot, S.out);
  HIPCHK(c, hipGetLastError());
  if (zip) return gz_run(c, who, S.out, off, ns, bytes, cap, gz_off, need);
  if ((rc = mark(4))) return rc;
  HIPCHK(c, hipMemcpyAsync(bytes, S.out, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  if ((rc = mark(5))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (!denovo) { S.clk.set(2, 3, 4); S.clk.set(3, 4, 5); }
  return SMR_OK;
}
}  // namespace
extern "C" int smr_fastx_split(smr_ctx* c, int mates, const smr_fxsplit_opts* o, const uint8_t* hit, uint8_t* bytes, uint64_t cap, uint64_t off[9], uint64_t* need) {
  return fxs_impl(c, "smr_fastx_split", false, false, mates, o, hit, bytes, cap, off, nullptr, need);
}
extern "C" int smr_fastx_split_gz(smr_ctx* c, int mates, const smr_fxsplit_opts* o, const uint8_t* hit, uint8_t* gz, uint64_t cap, uint64_t gz_off[9], uint64_t plain_off[9],
                                  uint64_t* need) {
  return fxs_impl(c, "smr_fastx_split_gz", false, true, mates, o, hit, gz, cap, plain_off, gz_off, need);
}
extern "C" int smr_fastx_split_times(const smr_ctx* c, double ms[4]) {
  if (!c || !ms) return SMR_ERR_ARG;
  c->fxs.clk.copy_to(ms);
  return SMR_OK;
}
extern "C" int smr_fastx_denovo(smr_ctx* c, int mates, const smr_fxsplit_opts* o, const uint8_t* dn, uint8_t* bytes, uint64_t cap, uint64_t off[5], uint64_t* need) {
  return fxs_impl(c, "smr_fastx_denovo", true, false, mates, o, dn, bytes, cap, off, nullptr, need);
}
extern "C" int smr_fastx_denovo_gz(smr_ctx* c, int mates, const smr_fxsplit_opts* o, const uint8_t* dn, uint8_t* gz, uint64_t cap, uint64_t gz_off[5], uint64_t plain_off[5],
                                   uint64_t* need) {
  return fxs_impl(c, "smr_fastx_denovo_gz", true, true, mates, o, dn, gz, cap, plain_off, gz_off, need);
}
