// smr_score_text.hpp -- host only: e-value and bit score of an alignment as the BLAST reports print them (report_blast.cpp:118-125).  They
// depend on the database and score1 only.  The one definition for the report writer (smr_report.cpp: add_rows) and for the table
// smr_rows_part hands its kernels (smr_engine_rows.hpp): same expressions, same stream settings.
#pragma once
#include <cmath>
#include <cstdint>
#include <sstream>
#include <string>

namespace smr {
inline void score_texts(double lambda, double K, uint64_t full_ref, uint64_t full_read, uint32_t score1, std::string& evalue_text, std::string& bitscore_text) {
  const uint16_t s1 = (uint16_t)score1;
  const uint32_t bitscore = (uint32_t)((float)(lambda * s1 - std::log(K)) / (float)std::log(2));
  const double evalue = (double)K * full_ref * full_read * std::exp(-lambda * s1);
  std::ostringstream se, sb;
  se.precision(3);
  se << evalue;
  sb << bitscore;
  evalue_text = se.str(); bitscore_text = sb.str();
}
}  // namespace smr
