// mates_host_loop.cpp -- measurement aid of tools/mates_rows_cost.py (not part of the library): the per-pair loop that writes the SAM / BLAST rows
// or the pairwise text of mates in two reads files on the host, as examples/smr_align.cpp runs it under --mates host, in native code so that
// the tool times the loop and not an interpreter.  smr_results_fetch of both batches (batch 0 is selected again at the end), then per pair
// smr_reads_record_text twice per mate (sizes, then the three strings), smr_result_record_batch twice per mate and smr_report_add_pair.
#include <cstdint>
#include <vector>

#include "smr_hip.h"

namespace {
struct Mate { std::vector<char> h, s, q; std::vector<uint8_t> rec; };
int load(const smr_ctx* gpu, int batch, const smr_reads* reads, uint32_t i, Mate& m) {
  size_t tl[3];
  const int rc = smr_reads_record_text(reads, i, nullptr, 0, nullptr, 0, nullptr, 0, tl);
  if (rc != SMR_OK) return rc;
  m.h.resize(tl[0] + 1); m.s.resize(tl[1] + 1); m.q.resize(tl[2] + 1);
  smr_reads_record_text(reads, i, m.h.data(), m.h.size(), m.s.data(), m.s.size(), m.q.data(), m.q.size(), tl);
  const size_t len = smr_result_record_batch(gpu, batch, i, nullptr, 0);
  m.rec.resize(len);
  if (len) smr_result_record_batch(gpu, batch, i, m.rec.data(), len);
  return SMR_OK;
}
}  // namespace

extern "C" int mates_host_loop(smr_ctx* gpu, const smr_reads* reads1, const smr_reads* reads2, smr_report* rep, int is_fastq) {
  int rc;
  for (int b = 1; b >= 0; b--)
    if ((rc = smr_batch_select(gpu, b)) != SMR_OK || (rc = smr_results_fetch(gpu)) != SMR_OK) return rc;
  Mate m1, m2;
  const uint32_t n = smr_reads_count(reads1);
  for (uint32_t i = 0; i < n; i++) {
    if ((rc = load(gpu, 0, reads1, i, m1)) != SMR_OK || (rc = load(gpu, 1, reads2, i, m2)) != SMR_OK) return rc;
    if ((rc = smr_report_add_pair(rep, m1.h.data(), m1.s.data(), is_fastq ? m1.q.data() : nullptr, m1.rec.data(), m1.rec.size(),
                                  m2.h.data(), m2.s.data(), is_fastq ? m2.q.data() : nullptr, m2.rec.data(), m2.rec.size())) != SMR_OK) return rc;
  }
  return SMR_OK;
}
