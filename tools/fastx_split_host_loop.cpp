// fastx_split_host_loop.cpp -- measurement aid of tools/fastx_split_cost.py (not part of the library): the per-read loop that writes
// aligned.* / other.* on the host, as examples/smr_align.cpp runs it under --split host, in native code so that the tool times the loop and
// not an interpreter.  smr_results_fetch, then per read smr_reads_record_text twice (sizes, then the three strings) and smr_report_add with
// the read's record: `hit_record` for the reads whose hit byte is set, none for the others.
#include <cstdint>
#include <vector>

#include "smr_hip.h"

extern "C" int fxs_host_loop(smr_ctx* gpu, const smr_reads* reads, smr_report* rep, int is_fastq, const uint8_t* hit, const uint8_t* hit_record, uint64_t hit_record_len) {
  int rc = smr_results_fetch(gpu);
  if (rc != SMR_OK) return rc;
  std::vector<char> h, s, q;
  const uint32_t n = smr_reads_count(reads);
  for (uint32_t i = 0; i < n; i++) {
    size_t tl[3];
    if ((rc = smr_reads_record_text(reads, i, nullptr, 0, nullptr, 0, nullptr, 0, tl)) != SMR_OK) return rc;
    h.resize(tl[0] + 1); s.resize(tl[1] + 1); q.resize(tl[2] + 1);
    smr_reads_record_text(reads, i, h.data(), h.size(), s.data(), s.size(), q.data(), q.size(), tl);
    if ((rc = smr_report_add(rep, h.data(), s.data(), is_fastq ? q.data() : nullptr, hit[i] ? hit_record : nullptr, hit[i] ? (size_t)hit_record_len : 0)) != SMR_OK) return rc;
  }
  return SMR_OK;
}
