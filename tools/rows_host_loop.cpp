// rows_host_loop.cpp -- measurement aid of tools/rows_cost.py (not part of the library): the per-read loop that writes the SAM and BLAST rows on
// the host, as examples/smr_align.cpp runs it under --rows host, in native code so that the tool times the loop and not an interpreter.
// smr_results_fetch, then per read smr_reads_record_text twice (sizes, then the three strings), smr_result_record twice and smr_report_add.
#include <cstdint>
#include <vector>

#include "smr_hip.h"

extern "C" int rows_host_loop(smr_ctx* gpu, const smr_reads* reads, smr_report* rep, int is_fastq) {
  int rc = smr_results_fetch(gpu);
  if (rc != SMR_OK) return rc;
  std::vector<char> h, s, q;
  std::vector<uint8_t> rec;
  const uint32_t n = smr_reads_count(reads);
  for (uint32_t i = 0; i < n; i++) {
    size_t tl[3];
    if ((rc = smr_reads_record_text(reads, i, nullptr, 0, nullptr, 0, nullptr, 0, tl)) != SMR_OK) return rc;
    h.resize(tl[0] + 1); s.resize(tl[1] + 1); q.resize(tl[2] + 1);
    smr_reads_record_text(reads, i, h.data(), h.size(), s.data(), s.size(), q.data(), q.size(), tl);
    const size_t len = smr_result_record(gpu, i, nullptr, 0);
    rec.resize(len);
    if (len) smr_result_record(gpu, i, rec.data(), len);
    if ((rc = smr_report_add(rep, h.data(), s.data(), is_fastq ? q.data() : nullptr, rec.data(), len)) != SMR_OK) return rc;
  }
  return SMR_OK;
}
