// smr_engine_import.hpp -- host side of the state import (included by smr_engine.hip; kernel in smr_import.hpp): smr_state_import,
// smr_counters_import.  The reference restores every read from its key-value store at the start of every (index, part) (Read::load_db,
// read.cpp:467-539, called from align2(), processor.cpp:116-126); here the stored state of a batch lives in d_saved / d_saved_aln / the CIGAR
// pool, k_begin_part starts every part from them, and filling them from record bytes resumes a run that another process left off.

namespace {
// the per-read stored state of B as an upload leaves it, without a write to d_saved / d_saved_aln when the caller rewrites them anyway; the
// Readstats counters (num_aligned, num_short, reads_matched_per_db) stay: they are smr_counters_import's
int import_fresh(smr_ctx* c, Batch& B, bool clear_saved) {
  B.gen++;
  if (clear_saved) {
    HIPCHK(c, hipMemsetAsync(B.d_saved, 0, (size_t)B.n * sizeof(RState), c->stream));
    HIPCHK(c, hipMemsetAsync(B.d_saved_aln, 0, (size_t)B.n * B.slots * sizeof(AlignRec), c->stream));
  }
  HIPCHK(c, hipMemsetAsync(B.d_ctr + C_ERR_HITCAP, 0, (size_t)(C_SW_SPEC - C_ERR_HITCAP) * 8, c->stream));      // error flags and cursors, C_CIGAR_CURSOR among them
  HIPCHK(c, hipMemsetAsync(B.d_ctr + C_PCUR, 0, (size_t)C_NSHARD * C_PCUR_STRIDE * 8, c->stream));
  HIPCHK(c, hipMemsetAsync(B.d_ctr + C_IDCOV, 0, 4 * 8, c->stream));
  if (B.d_idcov) HIPCHK(c, hipMemsetAsync(B.d_idcov, 0, std::min(B.d_idcov.cap() / 4, (size_t)B.n) * 16, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  B.fetched = false;
  return SMR_OK;
}
}  // namespace

extern "C" int smr_state_import(smr_ctx* c, const uint8_t* bytes, const uint64_t* off, uint32_t n) {
  if (!c) return SMR_ERR_ARG;
  Batch& B = *c->b;
  if (!B.d_saved) { set_err(c, "smr_state_import: no reads uploaded"); return SMR_ERR_STATE; }
  if (B.idcov_ran) { set_err(c, "smr_state_import after smr_idcov_part: the id / coverage pass has counted alignments of this batch; smr_state_reset or upload first"); return SMR_ERR_STATE; }
  HIPCHK(c, hipSetDevice(c->device));
  ev_drop(c);
  int rc;
  // nothing of a refused import stays: the batch is as an upload leaves it, the message is the refusal's
  auto refuse = [&](int code, const std::string& why) -> int {
    if (import_fresh(c, B, true) == SMR_OK) set_err(c, why);
    return code;
  };
  if (!off) return refuse(SMR_ERR_ARG, "smr_state_import: null offsets");
  if (n != B.n) return refuse(SMR_ERR_ARG, "smr_state_import: " + std::to_string(n) + " records for a batch of " + std::to_string(B.n) + " reads");
  if (off[0] > off[n]) return refuse(SMR_ERR_ARG, "smr_state_import: offsets must not decrease");
  const uint64_t o_base = off[0], total = off[n] - off[0];           // (off[0] need not be 0: a slice of a larger set of records)
  if (total && !bytes) return refuse(SMR_ERR_ARG, "smr_state_import: null record bytes");
  if (total / 4 >= 0xFFFFFFF0ull) return refuse(SMR_ERR_CAPACITY, "smr_state_import: the records can hold more CIGAR words than the pool's limit of 2^32");
  if ((rc = import_fresh(c, B, false))) return rc;
  if (n == 0) return SMR_OK;
  // the CIGAR pool: whatever it held is replaced, and all CIGAR words of the records together are fewer than a quarter of their bytes
  const uint64_t need = total / 4;
  if (need > B.cigar_words) {
    const uint64_t w = std::max<uint64_t>(need, 1u << 20);
    if ((rc = B.d_cigar.alloc(c, (size_t)w))) { B.cigar_words = 0; return rc; }
    B.cigar_words = w;
  }
  DevBuf<uint32_t> d_bytes, d_flag; DevBuf<unsigned long long> d_off;      // (of this call)
  uint32_t h_flag[4] = {0, 0, 0, 0};
  auto run = [&]() -> int {
    int r2;
    const size_t nw = (size_t)((total + 3) / 4);
    if ((r2 = d_bytes.alloc(c, nw + 2)) || (r2 = d_off.alloc(c, (size_t)n + 1)) || (r2 = d_flag.alloc(c, 4))) return r2;
    HIPCHK(c, hipMemsetAsync(d_bytes + (nw ? nw - 1 : 0), 0, 8, c->stream));          // the last word ends on bytes that are not the caller's
    if (total) HIPCHK(c, hipMemcpyAsync(d_bytes, bytes + o_base, (size_t)total, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_off, off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_flag, 0, 16, c->stream));
    const uint32_t chunks = (n + 63u) / 64u, blocks = std::min<uint32_t>((chunks + 3u) / 4u, (uint32_t)c->n_cu * 8u);
    launch(c, k_import_state, dim3(blocks), dim3(256), 0, (const uint32_t*)d_bytes, (unsigned long long)o_base, (unsigned long long)total, (const unsigned long long*)d_off, n, B.slots,
                       (const uint32_t*)B.d_len, B.d_saved, B.d_saved_aln, B.d_cigar, (unsigned long long)B.cigar_words, B.d_ctr, d_flag);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_flag, d_flag, 16, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SMR_OK;
  };
  rc = run();
  (void)hipStreamSynchronize(c->stream);
  d_bytes.release(); d_off.release(); d_flag.release();
  if (rc == SMR_OK && h_flag[0]) {
    const uint32_t f = h_flag[0];
    if (f & (IMP_ERR_FORMAT | IMP_ERR_POOL)) return refuse(SMR_ERR_ARG, "smr_state_import: a record's lengths (alignment_size, an alignment's length or its CIGAR length) do not add up to the bytes given for it");
    if (f & IMP_ERR_SLOTS) return refuse(SMR_ERR_CAPACITY, "smr_state_import: a record holds more alignments than max_alignments_per_read (smr_reads_upload)");
    if (f & IMP_ERR_READLEN) return refuse(SMR_ERR_ARG, "smr_state_import: an alignment's readlen differs from the length of the uploaded read (records of other reads?)");
    if (f & IMP_ERR_IDCOV) return refuse(SMR_ERR_ARG, "smr_state_import: a record carries id / coverage counters; resuming after smr_idcov_part is not supported");
    return refuse(SMR_ERR_ARG, "smr_state_import: the records disagree on num_alignments");
  }
  if (rc != SMR_OK) {                                       // a device error: its message stays
    std::string why; { std::lock_guard<std::mutex> l_(c->err_m); why = c->err; }
    return refuse(rc, why);
  }
  if (h_flag[3]) B.last_num_alignments = h_flag[2];         // Read::num_alignments of the records (what smr_result_record writes back)
  return SMR_OK;
}

extern "C" int smr_counters_import(smr_ctx* c, const uint64_t* in, uint32_t n_db) {
  if (!c || !in) return SMR_ERR_ARG;
  Batch& B = *c->b;
  if (!B.d_saved || !B.d_ctr) { set_err(c, "smr_counters_import: no reads uploaded"); return SMR_ERR_STATE; }
  if (B.idcov_ran) { set_err(c, "smr_counters_import after smr_idcov_part; smr_state_reset or upload first"); return SMR_ERR_STATE; }
  if (n_db > 64) { set_err(c, "smr_counters_import: n_db must be <= 64"); return SMR_ERR_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  unsigned long long h[C_PER_DB + 64];
  memset(h, 0, sizeof h);
  h[C_NUM_ALIGNED] = in[0]; h[C_NUM_SHORT] = in[1];
  for (uint32_t i = 0; i < n_db; i++) h[C_PER_DB + i] = in[2 + i];
  HIPCHK(c, hipMemcpyAsync(B.d_ctr, h, sizeof h, hipMemcpyHostToDevice, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SMR_OK;
}
