// smr_engine_export.hpp -- host side of the state export (included by smr_engine.hip; kernels in smr_export.hpp): smr_state_export, the
// counterpart of smr_state_import.  The records of the selected batch are sized and serialised on the device (what record_of does on the
// host one read at a time after smr_results_fetch) and cross the bus once, as the bytes a key-value writer or a state file takes.

extern "C" int smr_state_export(smr_ctx* c, uint8_t* bytes, uint64_t cap, uint64_t* off, uint32_t n, uint64_t* need) {
  if (!c) return SMR_ERR_ARG;
  Batch& B = *c->b;
  if (!B.d_saved) { set_err(c, "smr_state_export: no reads uploaded"); return SMR_ERR_STATE; }
  if (n != B.n) { set_err(c, "smr_state_export: n = " + std::to_string(n) + " for a batch of " + std::to_string(B.n) + " reads"); return SMR_ERR_ARG; }
  HIPCHK(c, hipSetDevice(c->device));
  if (need) *need = 0;
  if (n == 0) { if (off) off[0] = 0; return SMR_OK; }
  int rc;
  const uint32_t np = (n + EXP_SIZE_BLOCK - 1u) / EXP_SIZE_BLOCK;
  if (c->d_xoff.cap() < (size_t)n + 1) {                     // (both or neither: d_xoff's capacity stands for the pair)
    if ((rc = c->d_xoff.alloc(c, (size_t)n + 1)) || (rc = c->d_xpart.alloc(c, (size_t)np))) { c->d_xoff.release(); return rc; }
  }
  launch(c, k_export_size, dim3(np), dim3(EXP_SIZE_BLOCK), 0, n, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, c->d_xoff, c->d_xpart);
  if (np > 1) {
    launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, c->d_xpart, np);
    launch(c, k_export_offsets, dim3(np), dim3(EXP_SIZE_BLOCK), 0, n, c->d_xoff, (const unsigned long long*)c->d_xpart);
  }
  HIPCHK(c, hipGetLastError());
  unsigned long long total = 0;
  HIPCHK(c, hipMemcpyAsync(&total, c->d_xoff + n, 8, hipMemcpyDeviceToHost, c->stream));
  if (off) HIPCHK(c, hipMemcpyAsync(off, c->d_xoff, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (need) *need = total;
  if (!bytes) return SMR_OK;
  if (cap < total) { set_err(c, "smr_state_export: the records take " + std::to_string(total) + " bytes, the buffer has " + std::to_string(cap)); return SMR_ERR_CAPACITY; }
  if (total == 0) return SMR_OK;
  if ((rc = c->d_xbytes.reserve_headroom(c, (size_t)total, 0))) return rc;
  const uint32_t chunks = (n + 63u) / 64u, blocks = std::min<uint32_t>((chunks + 3u) / 4u, (uint32_t)c->n_cu * 8u);
  launch(c, k_export_state, dim3(blocks), dim3(256), 0, n, B.slots, (const RState*)B.d_saved, (const AlignRec*)B.d_saved_aln, (const uint32_t*)B.d_cigar,
                     (unsigned long long)(B.d_cigar ? B.cigar_words : 0), (const uint32_t*)B.d_idcov, B.last_num_alignments, (const unsigned long long*)c->d_xoff, c->d_xbytes);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipMemcpyAsync(bytes, c->d_xbytes, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return SMR_OK;
}
