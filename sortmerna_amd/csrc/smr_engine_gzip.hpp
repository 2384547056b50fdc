// smr_engine_gzip.hpp -- host side of the DEFLATE kernels (smr_gzip.hpp; included by smr_engine.hip): gz_run, the dispatcher that turns byte
// ranges of a device buffer into gzip members and copies only those to the host, and smr_gzip_batch / smr_gzip_lines_batch, the same over a
// host buffer (building blocks and the tests' seam).  smr_fastx_split_gz / smr_fastx_denovo_gz (smr_engine_fxsplit.hpp) hand it the streams
// their plain siblings would have copied back; smr_rows_part_gz and smr_pairwise_part_gz (smr_engine_rows.hpp, smr_engine_pairwise.hpp) do so
// with the chunks cut at line ends.
//
// The tokens of a chunk take four bytes per plain byte, so the chunks are worked on in rounds of GZ_ROUND; the members wait in worst-case
// slots (the stored form's size) until all sizes are known, then one scan and one compaction put them back to back.

namespace {
#define GZ_ROUND 1024u           // chunks per round: 256 MiB of tokens

// the CRC-32 byte table (reflected, 0xEDB88320) and, for k = 0 .. 7, the GF(2) operator "the register after 2^k slices of zero bytes"
void gz_crc_words(uint32_t* w) {
  for (uint32_t i = 0; i < 256u; i++) {
    uint32_t x = i;
    for (int k = 0; k < 8; k++) x = (x & 1u) ? 0xEDB88320u ^ (x >> 1) : x >> 1;
    w[i] = x;
  }
  uint32_t m[32], q[32];
  for (uint32_t k = 0; k < 32u; k++) m[k] = w[(1u << k) & 0xFFu] ^ ((1u << k) >> 8);      // one zero byte
  auto square = [&]() {
    for (uint32_t k = 0; k < 32u; k++) { uint32_t y = 0; for (uint32_t b = 0; b < 32u; b++) if ((m[k] >> b) & 1u) y ^= m[b]; q[k] = y; }
    memcpy(m, q, sizeof m);
  };
  uint32_t bytes = 1;
  while (bytes < GZ_SLICE) { square(); bytes *= 2u; }
  for (uint32_t k = 0; k < 8u; k++) { memcpy(w + 256u + 32u * k, m, sizeof m); square(); }
}

// the table on the device, made at its first use (by the compressor, or by the decoder of smr_engine_gunzip.hpp on either stream)
int gz_crc_table(smr_ctx* c, hipStream_t st) {
  std::lock_guard<std::mutex> l_(c->gz_tab_m);
  if (c->gz.crc_tab) return SMR_OK;
  uint32_t w[GZ_CRC_WORDS];
  gz_crc_words(w);
  int rc;
  if ((rc = c->gz.crc_tab.alloc(c, GZ_CRC_WORDS))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->gz.crc_tab, w, sizeof w, hipMemcpyHostToDevice, st));
  HIPCHK(c, hipStreamSynchronize(st));                 // (w leaves the scope)
  return SMR_OK;
}

// n_streams ranges [off[k], off[k + 1]) of d_in -> their gzip members, back to back, in gz (may be null: sizes only); gz_off[n_streams + 1].
// The two forms differ in the chunk table only.  lines = false: a chunk every GZ_CHUNK bytes of a stream; the table is made here and uploaded.
// lines = true: the fixed grid of k_gz_cut_lines, which writes the table where it is used, and one scan on the device turns the slot sizes it
// leaves into the slot offsets -- no cut crosses the bus; the slots are reserved for what the chunks can take at the most (their plain bytes
// and, a chunk of this form being shorter than 65 536 bytes, the 30 bytes of gz_slot_size over them).  Everything behind the table is one body
int gz_run(smr_ctx* c, const char* who, const uint8_t* d_in, const uint64_t* off, uint32_t n_streams, uint8_t* gz, uint64_t cap, uint64_t* gz_off, uint64_t* need,
           bool lines = false) {
  GzScratch& S = c->gz;
  int rc;
  if ((rc = S.clk.begin(c))) return rc;
  for (uint32_t k = 0; k <= n_streams; k++) gz_off[k] = 0;
  if (need) *need = 0;
  std::vector<GzChunk> chunks;
  std::vector<unsigned long long> slot_off, cut_tab;   // cut_tab: off[], then first[], as k_gz_cut_lines reads them
  std::vector<uint64_t> first(n_streams + 1u);
  unsigned long long slots_bytes = 0;
  uint64_t n_chunks = 0;
  for (uint32_t k = 0; k < n_streams; k++) {
    first[k] = n_chunks;
    if (lines) { n_chunks += (off[k + 1] - off[k] + GZ_LINE_PITCH - 1u) / GZ_LINE_PITCH; continue; }
    for (uint64_t at = off[k]; at < off[k + 1]; at += GZ_CHUNK) {
      GzChunk ck; ck.src = at; ck.len = (uint32_t)std::min<uint64_t>(GZ_CHUNK, off[k + 1] - at); ck.pad = 0;
      chunks.push_back(ck); slot_off.push_back(slots_bytes);
      slots_bytes += gz_slot_size(ck.len);
      n_chunks++;
    }
  }
  first[n_streams] = n_chunks;
  if (n_chunks == 0) return SMR_OK;
  if (n_chunks >= 0x7FFFFFFFull) { set_err(c, std::string(who) + ": 2^31 - 1 chunks or more"); return SMR_ERR_CAPACITY; }
  const uint32_t nc = (uint32_t)n_chunks, round = std::min(nc, GZ_ROUND);
  if (lines) slots_bytes = (off[n_streams] - off[0]) + 30ull * nc;
  if ((rc = gz_crc_table(c, c->stream))) return rc;
  if ((rc = S.chunks.reserve(c, nc)) || (rc = S.slot_off.reserve(c, nc)) || (rc = S.sizes.reserve(c, (size_t)nc + 1u)) || (rc = S.codes.reserve(c, nc)) ||
      (rc = S.crc.reserve(c, nc)) || (rc = S.tok.reserve(c, (size_t)round * GZ_TOK_STRIDE)) || (rc = S.freq.reserve(c, (size_t)round * GZ_FREQ_STRIDE)) ||
      (rc = S.ntok.reserve(c, round))) return rc;
  if (gz && (rc = S.slots.reserve(c, (size_t)slots_bytes))) return rc;
  if (lines) {
    cut_tab.assign(off, off + n_streams + 1u);
    cut_tab.insert(cut_tab.end(), first.begin(), first.end());
    if ((rc = S.cut_tab.reserve(c, cut_tab.size()))) return rc;
    HIPCHK(c, hipMemcpyAsync(S.cut_tab, cut_tab.data(), cut_tab.size() * 8u, hipMemcpyHostToDevice, c->stream));
  } else {
    HIPCHK(c, hipMemcpyAsync(S.chunks, chunks.data(), (size_t)nc * sizeof(GzChunk), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(S.slot_off, slot_off.data(), (size_t)nc * 8u, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(c, hipMemsetAsync(S.sizes + nc, 0, 8, c->stream));
  for (uint32_t b = 0; b < nc; b += round) {
    const uint32_t m = std::min(round, nc - b);
    if ((rc = S.clk.mark(c, 0, c->stream))) return rc;
    if (lines && b == 0) {                             // (timed with the matching of the first round)
      launch(c, k_gz_cut_lines, dim3(nc), dim3(256), 0, d_in, (const unsigned long long*)S.cut_tab, (const unsigned long long*)(S.cut_tab + n_streams + 1u), n_streams,
             (GzChunk*)S.chunks, (unsigned long long*)S.slot_off);
      launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.slot_off, nc);
    }
    launch(c, k_gz_match, dim3(m), dim3(GZ_WIN), 0, d_in, (const GzChunk*)(S.chunks + b), (const uint32_t*)S.crc_tab, S.tok, S.freq, S.ntok, S.crc + b);
    if ((rc = S.clk.mark(c, 1, c->stream))) return rc;
    launch(c, k_gz_codes, dim3(m), dim3(64), 0, (const GzChunk*)(S.chunks + b), (const uint32_t*)S.freq, S.codes + b, S.sizes + b);
    if ((rc = S.clk.mark(c, 2, c->stream))) return rc;
    // (sizes only: the sizes are known once the codes are; the members themselves are not made)
    if (gz) launch(c, k_gz_encode, dim3(m), dim3(256), 0, d_in, (const GzChunk*)(S.chunks + b), (const uint32_t*)S.tok, (const uint32_t*)S.ntok, (const uint32_t*)(S.crc + b),
                   (const GzCode*)(S.codes + b), (const unsigned long long*)(S.slot_off + b), S.slots);
    HIPCHK(c, hipGetLastError());
    if ((rc = S.clk.mark(c, 3, c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));        // the next round takes the token arrays (and the events)
    S.clk.add(0, 0, 1);
    S.clk.add(1, 1, 2);
    S.clk.add(2, 2, 3);
  }
  if ((rc = S.clk.mark(c, 0, c->stream))) return rc;
  launch(c, k_export_scan, dim3(1), dim3(EXP_SIZE_BLOCK), 0, S.sizes, nc + 1u);
  HIPCHK(c, hipGetLastError());
  std::vector<unsigned long long> excl((size_t)nc + 1u);
  HIPCHK(c, hipMemcpyAsync(excl.data(), S.sizes, ((size_t)nc + 1u) * 8u, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  for (uint32_t k = 0; k <= n_streams; k++) gz_off[k] = excl[first[k]];
  const uint64_t total = excl[nc];
  if (need) *need = total;
  if (!gz) return SMR_OK;
  if (cap < total) { set_err(c, std::string(who) + ": the members take " + std::to_string(total) + " bytes, the buffer has " + std::to_string(cap)); return SMR_ERR_CAPACITY; }
  if ((rc = S.out.reserve(c, (size_t)((total + 4095u) & ~4095ull)))) return rc;
  launch(c, k_gz_compact, dim3(nc), dim3(256), 0, (const GzCode*)S.codes, (const unsigned long long*)S.slot_off, (const uint8_t*)S.slots, (const unsigned long long*)S.sizes, S.out);
  HIPCHK(c, hipGetLastError());
  if ((rc = S.clk.mark(c, 1, c->stream))) return rc;
  HIPCHK(c, hipMemcpyAsync(gz, S.out, (size_t)total, hipMemcpyDeviceToHost, c->stream));
  if ((rc = S.clk.mark(c, 2, c->stream))) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  S.clk.set(3, 0, 1);
  S.clk.set(4, 1, 2);
  return SMR_OK;
}
}  // namespace

extern "C" uint32_t smr_gzip_chunk(void) { return GZ_CHUNK; }
extern "C" uint64_t smr_gzip_bound(uint64_t plain_bytes, uint64_t n_chunks) {
  // per member 18 + its plain bytes + 5 per stored block of at most 65 535 bytes: one block per member, and a further one in every member that
  // is a whole chunk -- of which plain_bytes allow plain_bytes / GZ_CHUNK.  For the chunks of one stream this is the sum over its members.
  const uint64_t per_full = (GZ_CHUNK + 65534u) / 65535u;
  return 18u * n_chunks + plain_bytes + 5u * (n_chunks + (per_full - 1u) * std::min<uint64_t>(n_chunks, plain_bytes / GZ_CHUNK));
}
namespace {
// smr_gzip_batch and smr_gzip_lines_batch: the streams go to the device, gz_run does the rest
int gz_batch(smr_ctx* c, const char* who, bool lines, const uint8_t* plain, const uint64_t* off, uint32_t n_streams, uint8_t* gz, uint64_t cap, uint64_t* gz_off, uint64_t* need) {
  if (!c || !off || !gz_off || !need) return SMR_ERR_ARG;
  for (uint32_t k = 0; k <= n_streams; k++) gz_off[k] = 0;
  *need = 0;
  for (uint32_t k = 0; k < n_streams; k++) if (off[k + 1] < off[k]) { set_err(c, std::string(who) + ": the offsets decrease"); return SMR_ERR_ARG; }
  const uint64_t n = off[n_streams] - off[0];
  if (n == 0) return SMR_OK;
  if (!plain) return SMR_ERR_ARG;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  if ((rc = c->gz.in.reserve(c, (size_t)n))) return rc;
  HIPCHK(c, hipMemcpyAsync(c->gz.in, plain + off[0], (size_t)n, hipMemcpyHostToDevice, c->stream));
  std::vector<uint64_t> rel(n_streams + 1u);
  for (uint32_t k = 0; k <= n_streams; k++) rel[k] = off[k] - off[0];
  return gz_run(c, who, c->gz.in, rel.data(), n_streams, gz, cap, gz_off, need, lines);
}
}  // namespace
extern "C" int smr_gzip_batch(smr_ctx* c, const uint8_t* plain, const uint64_t* off, uint32_t n_streams, uint8_t* gz, uint64_t cap, uint64_t* gz_off, uint64_t* need) {
  return gz_batch(c, "smr_gzip_batch", false, plain, off, n_streams, gz, cap, gz_off, need);
}
extern "C" uint64_t smr_gzip_lines_bound(uint64_t plain_bytes, uint32_t n_streams) {
  // a stream of n bytes has ceil(n / GZ_LINE_PITCH) members, one more than n / GZ_LINE_PITCH at the most
  return smr_gzip_bound(plain_bytes, plain_bytes / GZ_LINE_PITCH + n_streams);
}
extern "C" int smr_gzip_lines_batch(smr_ctx* c, const uint8_t* plain, const uint64_t* off, uint32_t n_streams, uint8_t* gz, uint64_t cap, uint64_t* gz_off, uint64_t* need) {
  return gz_batch(c, "smr_gzip_lines_batch", true, plain, off, n_streams, gz, cap, gz_off, need);
}
extern "C" int smr_gzip_times(const smr_ctx* c, double ms[5]) {
  if (!c || !ms) return SMR_ERR_ARG;
  c->gz.clk.copy_to(ms);
  return SMR_OK;
}
