// smr_align.cpp -- a C++17 host driver over the C ABI of libsmr_hip (include/smr_hip.h): the shape of the reference's
// align() (/root/reference/src/sortmerna/processor.cpp:173-285) with the N x align2() thread loop of every (index, part)
// replaced by one batched GPU call, for one or more --ref databases.  It writes what the reference keeps in its KVDB:
//   <out>/records.bin   u64 n, then n x (u64 klen, key "0_<i>", u64 vlen, Read::toBinString bytes)   (reads with a record only)
//   <out>/summary.txt   total reads, reads passing the E-value threshold, per-DB counts, too-short reads
// and, on request, the reference's reports through smr_report_* (aligned/other FASTX, BLAST tabular, SAM):
//   --fastx --other --blast "1 cigar qcov qstrand" --sam
// --pack device: the reads files are parsed and 2-bit packed by kernels (smr_reads_upload_fastx_file) instead of by the host's cores; the
// default, --pack host, is smr_reads_load_fastx_text + smr_reads_upload.  Everything after that is the same, and so is every output file.
// --split device (needs --pack device): the text stays with the batches (SMR_FASTX_KEEP) and aligned.* / other.* are written from the streams
// of one smr_fastx_split call (smr_report_add_fastx) instead of read by read; the default, --split host, is smr_reads_record_text +
// smr_report_add / smr_report_add_pair.  Every output file is the same.
// --rows device (needs --pack device): the rows of aligned.sam and of the BLAST tabular report come from one smr_rows_part call per (index, part)
// (smr_report_add_rows) instead of read by read; the default, --rows host, is smr_report_add.  Single reads and interleaved mates; refused with
// --blast 0 (unless --pairwise device takes it) and with two reads files, whose rows stay with the host writer unless --mates device is given.  Every output file is the same.
// --pairwise device (needs --pack device and --blast 0): the BLAST pairwise text comes from one smr_pairwise_part call per (index, part)
// (smr_report_add_pairwise) instead of read by read; the default, --pairwise host, is smr_report_add.  Single reads and interleaved mates;
// refused with two reads files unless --mates device is given.  With --rows device and --split device the per-read loop feeds the report nothing.  Every output file is the same.
// -otu_map -de_novo_otu -id X -coverage X: the %id / %coverage pass (smr_idcov_part, the reference's denovo_stats) per (index, part) after all
// alignment, otu_map.txt and aligned_denovo.fa|fq, the two Results lines of aligned.log; defaults and refusals are the reference's.
// --mates device (needs two reads files and --rows device or --pairwise device): the rows and the pairwise text of mates in two files come from
// smr_rows_part_mates / smr_pairwise_part_mates (and, under --ziprows device, their _gz forms) with batch 0 selected and mates = 1, in the visit
// per (index, part) where the plain calls are made: the two batches' streams are interleaved on the device into the order of
// smr_report_add_pair.  The default, --mates host, keeps the refusals above.  Every output file is the same.
// --otu device (needs --pack device): the members of otu_map.txt come from one smr_otu_part call per (index, part) (smr_report_add_otu) and
// aligned_denovo.* from one smr_fastx_denovo call (smr_report_add_denovo) instead of read by read; the default, --otu host, is smr_report_add.
// Single reads and interleaved mates; refused with two reads files.  Every output file is the same.
// --otu-mates device (needs two reads files and --pack device): what --otu device does, for mates in two files: the members of otu_map.txt come
// from one smr_otu_part_mates call per (index, part) with batch 0 selected and mates = 1, in the visit that serves --rows device, and
// aligned_denovo.* from one smr_fastx_denovo call of layout 2.  With --split device and, for rows or pairwise text, --mates device, the per-pair
// loop feeds the report nothing.  The default, --otu-mates host, is smr_report_add_pair.  Every output file is the same.
// --zip device (needs --split device and gzipped reports): aligned.* / other.*, and with --otu device aligned_denovo.*, are deflated by the
// DEFLATE kernels where the split leaves them (smr_fastx_split_gz / smr_fastx_denovo_gz) and appended to the .gz files as gzip members
// (smr_report_add_fastx_gz / _add_denovo_gz); every file inflates to what --zip host writes.
// --ziprows device (needs --rows device or --pairwise device, and gzipped reports): the SAM / BLAST rows and the pairwise text are deflated
// where those calls leave them, in members that end at line ends (smr_rows_part_gz / smr_pairwise_part_gz), and kept by the report as gzip
// members until it closes (smr_report_add_rows_gz / _add_pairwise_gz); aligned.sam.gz and aligned.blast.gz inflate to what --ziprows host
// writes.  Independent of --split and --zip.
// --unzip device (needs --pack device): a gzip reads file goes to the device as it is and is inflated there by the DEFLATE decoder kernels
// (SMR_FASTX_INFLATE) instead of by zlib on one host thread; the default, --unzip host, and every output file stay as they are.
// Build:  g++ -std=c++17 -O2 examples/smr_align.cpp -Iinclude -Lsortmerna_amd/lib -lsmr_hip -Wl,-rpath,$PWD/sortmerna_amd/lib -o smr_align
// There is no CPU fallback: without a HIP device smr_create fails and the program exits like the reference does (ERR + exit 1).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <string>
#include <vector>

#include "smr_hip.h"

namespace {
[[noreturn]] void die(const std::string& m) { fprintf(stderr, "ERROR: %s\n", m.c_str()); exit(EXIT_FAILURE); }
struct Db { std::string fasta, idx_prefix; double lambda = 0, K = 0; bool has_gumbel = false; std::vector<smr_index*> parts; };
}  // namespace

int main(int argc, char** argv) {
  std::vector<Db> dbs;
  std::vector<std::string> reads_paths; std::string out_dir = ".";
  int zip_out = -1;                                         // -1: like the reads file (options.hpp zip_out, report_fx_base.cpp:94)
  smr_params base; smr_params_default(&base);
  double evalue = 1.0;
  int device = 0;
  bool pack_device = false, split_device = false, rows_device = false, pair_device = false, otu_device = false, otu_mates_device = false, zip_device = false, unzip_device = false, ziprows_device = false, mates_device = false;
  bool id_given = false, cov_given = false;
  smr_report_opts ro; memset(&ro, 0, sizeof ro);
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto val = [&]() -> std::string { if (i + 1 >= argc) die("missing value after " + a); return argv[++i]; };
    if (a == "-ref" || a == "--ref") { Db d; d.fasta = val(); dbs.push_back(d); }
    else if (a == "-idx" || a == "--idx") { if (dbs.empty()) die("--idx before --ref"); dbs.back().idx_prefix = val(); }   // reference-format index files
    else if (a == "-gumbel" || a == "--gumbel") { if (dbs.empty()) die("--gumbel before --ref"); dbs.back().lambda = atof(val().c_str()); dbs.back().K = atof(val().c_str()); dbs.back().has_gumbel = true; }
    else if (a == "-reads" || a == "--reads") { if (reads_paths.size() == 2) die("at most two --reads files (mates)"); reads_paths.push_back(val()); }
    else if (a == "-out" || a == "--out") out_dir = val();
    else if (a == "-e") evalue = atof(val().c_str());
    else if (a == "-num_alignments" || a == "--num_alignments") base.num_alignments = (uint32_t)atoi(val().c_str());
    else if (a == "-no-best" || a == "--no-best") base.is_best = 0;
    else if (a == "-min_lis" || a == "--min_lis") base.min_lis = atoi(val().c_str());
    else if (a == "-num_seeds" || a == "--num_seeds") base.num_seeds = atoi(val().c_str());
    else if (a == "-edges" || a == "--edges") base.edges = atoi(val().c_str());
    else if (a == "-full_search" || a == "--full_search") base.is_full_search = 1;
    else if (a == "-F") base.is_reverse = 0;
    else if (a == "-R") base.is_forward = 0;
    else if (a == "-match") base.match = atoi(val().c_str());
    else if (a == "-mismatch") { base.mismatch = atoi(val().c_str()); base.score_N = base.mismatch; }
    else if (a == "-gap_open") base.gap_open = atoi(val().c_str());
    else if (a == "-gap_ext") base.gap_ext = atoi(val().c_str());
    else if (a == "-device") device = atoi(val().c_str());
    else if (a == "-pack" || a == "--pack") { const std::string v = val(); if (v != "host" && v != "device") die("--pack: host or device"); pack_device = v == "device"; }
    else if (a == "-split" || a == "--split") { const std::string v = val(); if (v != "host" && v != "device") die("--split: host or device"); split_device = v == "device"; }
    else if (a == "-rows" || a == "--rows") { const std::string v = val(); if (v != "host" && v != "device") die("--rows: host or device"); rows_device = v == "device"; }
    else if (a == "-pairwise" || a == "--pairwise") { const std::string v = val(); if (v != "host" && v != "device") die("--pairwise: host or device"); pair_device = v == "device"; }
    else if (a == "-unzip" || a == "--unzip") { const std::string v = val(); if (v != "host" && v != "device") die("--unzip: host or device"); unzip_device = v == "device"; }
    else if (a == "-zip" || a == "--zip") { const std::string v = val(); if (v != "host" && v != "device") die("--zip: host or device"); zip_device = v == "device"; }
    else if (a == "-ziprows" || a == "--ziprows") { const std::string v = val(); if (v != "host" && v != "device") die("--ziprows: host or device"); ziprows_device = v == "device"; }
    else if (a == "-mates" || a == "--mates") { const std::string v = val(); if (v != "host" && v != "device") die("--mates: host or device"); mates_device = v == "device"; }
    else if (a == "-otu-mates" || a == "--otu-mates") { const std::string v = val(); if (v != "host" && v != "device") die("--otu-mates: host or device"); otu_mates_device = v == "device"; }
    else if (a == "-otu" || a == "--otu") { const std::string v = val(); if (v != "host" && v != "device") die("--otu: host or device"); otu_device = v == "device"; }
    else if (a == "-otu_map" || a == "--otu_map") ro.otu_map = 1;
    else if (a == "-de_novo_otu" || a == "--de_novo_otu") ro.denovo = 1;
    else if (a == "-id" || a == "--id") { ro.min_id = atof(val().c_str()); id_given = true; }
    else if (a == "-coverage" || a == "--coverage") { ro.min_cov = atof(val().c_str()); cov_given = true; }
    else if (a == "-fastx" || a == "--fastx") ro.fastx = 1;
    else if (a == "-other" || a == "--other") ro.other = 1;
    else if (a == "-sam" || a == "--sam") ro.sam = 1;
    else if (a == "-SQ" || a == "--SQ") ro.sam_sq = 1;
    else if (a == "-paired_in" || a == "--paired_in") ro.paired_in = 1;
    else if (a == "-paired_out" || a == "--paired_out") ro.paired_out = 1;
    else if (a == "-out2" || a == "--out2") ro.out2 = 1;
    else if (a == "-sout" || a == "--sout") ro.sout = 1;
    else if (a == "-zip-out" || a == "--zip-out") { const std::string v = val(); zip_out = (v == "1" || v == "true" || v == "t" || v == "yes" || v == "y") ? 1 : 0; }
    else if (a == "-blast" || a == "--blast") {            // "1" = tabular, optionally followed by cigar / qcov / qstrand (options.cpp opt_blast)
      const std::string v = val();
      if (v == "0") { ro.blast_pairwise = 1; continue; }   // BLAST-like pairwise text
      if (v.empty() || v[0] != '1') die("-blast: '0' (pairwise) or '1 [cigar] [qcov] [qstrand]' (tabular)");
      ro.blast_tabular = 1;
      const std::string cols = v.size() > 2 ? v.substr(2) : "";
      if (cols.size() >= sizeof ro.blast_cols) die("-blast: too many columns");
      strcpy(ro.blast_cols, cols.c_str());
    }
    else if (a == "-h" || a == "--help") {
      printf("usage: smr_align --ref DB.fasta --gumbel LAMBDA K [--idx PREFIX] [--ref ...] --reads READS.fa|fq[.gz] [--reads MATES] [--out DIR]\n"
             "       [-e EVALUE] [-num_alignments N] [-no-best] [-min_lis N] [-num_seeds N] [-edges N] [-full_search] [-F|-R]\n"
             "       [-match N -mismatch N -gap_open N -gap_ext N] [-device K] [--fastx] [--other] [--blast '0' | '1 cigar qcov qstrand'] [--sam [-SQ]]\n"
             "       [-zip-out 0|1] [--pack host|device] [--split host|device] [--zip host|device] [--ziprows host|device] [--unzip host|device] [--rows host|device] [--pairwise host|device] [--mates host|device] [-otu_map [-id X] [-coverage X]] [-de_novo_otu] [--otu host|device] [--otu-mates host|device] [-paired_in | -paired_out] [-out2] [-sout]     (two --reads files, or one interleaved file with -paired_in / -paired_out)\n");
      return 0;
    } else die("unknown option " + a);
  }
  if (mates_device && reads_paths.size() < 2) die("--mates device interleaves the rows of mates in two reads files on the device: it needs two --reads files");
  if (mates_device && !rows_device && !pair_device) die("--mates device interleaves what --rows device and --pairwise device write for two reads files: it needs one of the two");
  if (split_device && !pack_device) die("--split device writes aligned.* / other.* from the text the device parsed: it needs --pack device");
  if (unzip_device && !pack_device) die("--unzip device inflates a gzip reads file into the text buffer the device parses: it needs --pack device");
  if (rows_device && !pack_device) die("--rows device writes the SAM / BLAST rows from the text the device parsed: it needs --pack device");
  if (pair_device && !pack_device) die("--pairwise device writes the BLAST pairwise text from the text the device parsed: it needs --pack device");
  if (pair_device && !ro.blast_pairwise) die("--pairwise device writes the pairwise text of --blast 0: without --blast 0 there is none");
  if (pair_device && reads_paths.size() == 2 && !mates_device) die("--pairwise device takes one reads file (single reads or interleaved mates): the blocks of mates in two files alternate between the batches and stay with --pairwise host");
  if (rows_device && ro.blast_pairwise && !pair_device) die("--rows device writes BLAST tabular rows only: --blast 0 (pairwise) stays with --rows host");
  if (rows_device && reads_paths.size() == 2 && !mates_device) die("--rows device takes one reads file (single reads or interleaved mates): the rows of mates in two files alternate between the batches and stay with --rows host");
  // the reference's rules for the four options (options.cpp:1623-1628, 1667-1674, 1744-1757)
  if ((id_given || cov_given) && !ro.otu_map) die("options '-id' and '-coverage' can only be used together with '-otu_map': they are the thresholds of the OTU map");
  if (ro.otu_map && !base.is_best) die("option '-otu_map' cannot be used with '-no-best': the OTU map is built from the best alignments");
  if (ro.otu_map) { if (!id_given) ro.min_id = 0.97; if (!cov_given) ro.min_cov = 0.97; }
  if (!(ro.min_id >= 0 && ro.min_id <= 1 && ro.min_cov >= 0 && ro.min_cov <= 1)) die("-id and -coverage take a value within [0, 1]");
  const bool idcov = ro.otu_map || ro.denovo;
  if (otu_device && !pack_device) die("--otu device writes the OTU map and aligned_denovo.* from the text the device parsed: it needs --pack device");
  if (otu_device && reads_paths.size() == 2) die("--otu device takes one reads file (single reads or interleaved mates): the members of a group of mates in two files alternate between the batches and stay with --otu host");
  if (otu_mates_device && reads_paths.size() < 2) die("--otu-mates device writes the OTU map and aligned_denovo.* of mates in two reads files on the device: it needs two --reads files");
  if (otu_mates_device && !pack_device) die("--otu-mates device writes the OTU map and aligned_denovo.* from the text the device parsed: it needs --pack device");
  if (dbs.empty() || reads_paths.empty()) die("--ref and --reads are required (see --help)");
  if (const char* why = smr_params_refused(&base)) die(std::string("these options are outside what libsmr_hip aligns (the reference accepts them): ") + why);
  // minimal_score (which reads count as aligned) and the e-values / bit scores of the BLAST report depend on the Gumbel parameters of the
  // (scoring scheme, DB background) pair.  The reference computes them per DB with its vendored NCBI ALP library (refstats.cpp:194-233),
  // which is outside this library: they must be given -- from the reference's log ("Gumbel lambda = ..", "Gumbel K = ..") for the same DB
  // and the same -match/-mismatch/-gap_open/-gap_ext.  No default is assumed: a silent guess would classify a different set of reads.
  for (auto& d : dbs) if (!d.has_gumbel) die("--gumbel LAMBDA K is required after every --ref (see --help): the values of the reference's log for this DB and scoring scheme");
  if (zip_out == -1) {                                      // gzip reports for a gzip reads file
    unsigned char mg[2] = {0, 0};
    if (FILE* fz = fopen(reads_paths[0].c_str(), "rb")) { if (fread(mg, 1, 2, fz) != 2) mg[0] = 0; fclose(fz); }
    zip_out = (mg[0] == 0x1f && mg[1] == 0x8b) ? 1 : 0;
  }
  ro.zip_out = zip_out;
  if (zip_device && !split_device) die("--zip device compresses the aligned.* / other.* streams where --split device leaves them: it needs --split device");
  if (zip_device && !zip_out) die("--zip device writes gzip members: the reports of this run are not gzipped (a plain reads file without -zip-out 1, or -zip-out 0)");
  if (ziprows_device && !rows_device && !pair_device) die("--ziprows device compresses the SAM / BLAST rows and the pairwise text where --rows device and --pairwise device leave them: it needs one of the two");
  if (ziprows_device && !zip_out) die("--ziprows device writes gzip members: the reports of this run are not gzipped (a plain reads file without -zip-out 1, or -zip-out 0)");
  char err[512] = "";
  // reads (Readfeed::next -> Read::init, readfeed.hpp:124 / read.cpp:264-347)
  // (all cores parse and 2-bit pack the FASTA / FASTQ / .gz file; the text stays mapped for the report writers)
  // one batch per reads file (the second file holds the mates of the first: options.cpp:1591 is_paired)
  // (--pack device: the kernels of the engine do that, straight into batch b; what comes back has the text, the record offsets and the lengths)
  std::vector<smr_reads*> rf(reads_paths.size(), nullptr);
  uint64_t n = 0, total_len = 0; uint32_t min_len = 0xFFFFFFFFu, max_len = 0;
  smr_ctx* gpu = nullptr;
  const uint32_t slots = base.num_alignments > 0 ? base.num_alignments : 256;
  if (pack_device && smr_create(device, &gpu, err, sizeof err) != SMR_OK) die(err);
  for (size_t b = 0; b < rf.size(); b++) {
    if (pack_device) {
      if (smr_batch_select(gpu, (int)b) != SMR_OK) die(smr_last_error(gpu));
      if (smr_reads_upload_fastx_file(gpu, reads_paths[b].c_str(), slots, SMR_FASTX_VIEW | (unzip_device ? SMR_FASTX_INFLATE : 0u) | ((split_device || rows_device || pair_device || ((otu_device || otu_mates_device) && idcov)) ? SMR_FASTX_KEEP : 0u), &rf[b], err, sizeof err) != SMR_OK) die(err);
    } else if (smr_reads_load_fastx_text(reads_paths[b].c_str(), 0, &rf[b], err, sizeof err) != SMR_OK) die(err);
    n += smr_reads_count(rf[b]); total_len += smr_reads_total_len(rf[b]);
    if (smr_reads_count(rf[b])) { min_len = std::min(min_len, smr_reads_min_len(rf[b])); max_len = std::max(max_len, smr_reads_max_len(rf[b])); }
  }
  if (n == 0) min_len = 0;
  const bool is_fastq = smr_reads_is_fastq(rf[0]) != 0;
  const bool paired = rf.size() == 2 || ro.paired_in || ro.paired_out;
  if (rf.size() == 2 && smr_reads_count(rf[0]) != smr_reads_count(rf[1])) die("the two --reads files hold different numbers of reads");
  if (rf.size() == 1 && paired && (smr_reads_count(rf[0]) & 1)) die("-paired_in / -paired_out with one file: odd number of reads");

  // indexes: reference-built files when a prefix is given, else our own builder (Index ctor / build_index, index.cpp:61-107)
  for (auto& d : dbs) {
    if (!d.idx_prefix.empty()) {
      smr_index* p0 = nullptr;
      if (smr_index_load_files(d.idx_prefix.c_str(), 0, d.fasta.c_str(), &p0, err, sizeof err) != SMR_OK) die(err);
      smr_index_info info; smr_index_get_info(p0, &info);
      d.parts.push_back(p0);
      for (uint32_t k = 1; k < info.n_parts; k++) {
        smr_index* pk = nullptr;
        if (smr_index_load_files(d.idx_prefix.c_str(), k, d.fasta.c_str(), &pk, err, sizeof err) != SMR_OK) die(err);
        d.parts.push_back(pk);
      }
    } else {
      smr_index* arr[256]; uint32_t np = 0;
      if (smr_index_build(d.fasta.c_str(), 18, 3072.0, 10000, 0, arr, 256, &np, err, sizeof err) != SMR_OK) die(err);
      d.parts.assign(arr, arr + np);
    }
  }

  if (!gpu && smr_create(device, &gpu, err, sizeof err) != SMR_OK) die(err);
  if (smr_sw_mode(gpu, -1) == 0) fprintf(stderr, "smr_align: the 32-bit Smith-Waterman kernel is in use (packed kernel off or failed its self-check): expect about half the alignment rate\n");
  for (size_t b = 0; !pack_device && b < rf.size(); b++)
    if (smr_batch_select(gpu, (int)b) != SMR_OK || smr_reads_upload(gpu, rf[b], slots) != SMR_OK) die(smr_last_error(gpu));

  // the (index, part) loop of processor.cpp:219-277
  size_t n_parts_all = 0;
  for (auto& d : dbs) n_parts_all += d.parts.size();
  const bool rows_dev = rows_device && (ro.sam || ro.blast_tabular);
  const bool pair_dev = pair_device && !ro.blast_tabular;            // (with tabular rows as well the host writes no pairwise text either)
  const bool otu_dev = (otu_device || otu_mates_device) && idcov;       // (two reads files: --otu-mates device, the calls in their form for mates)
  const bool keep_part = (rows_dev || pair_dev || idcov) && n_parts_all == 1; // one part in all: it stays resident for the pass and for smr_rows_part / smr_pairwise_part / smr_otu_part
  for (size_t k = 0; k < dbs.size(); k++) {
    smr_index_info info; smr_index_get_info(dbs[k].parts[0], &info);
    smr_params p = base;
    p.minimal_score = smr_minimal_score(dbs[k].lambda, dbs[k].K, info.bg, info.full_len, info.numseq, n, total_len, evalue);
    p.index_num = (uint32_t)k;
    for (size_t part = 0; part < dbs[k].parts.size(); part++) {
      p.part = (uint32_t)part;
      p.is_last_index_part = (k + 1 == dbs.size() && part + 1 == dbs[k].parts.size());
      if (smr_index_upload(gpu, dbs[k].parts[part], 0) != SMR_OK) die(smr_last_error(gpu));
      for (size_t b = 0; b < rf.size(); b++) {
        if (smr_batch_select(gpu, (int)b) != SMR_OK || smr_align_part(gpu, 0, &p) != SMR_OK || smr_traceback(gpu, 0, &p) != SMR_OK) die(smr_last_error(gpu));
      }
      if (!keep_part) smr_index_unload(gpu, 0);
    }
  }
  // denovo_stats (processor.cpp:287-438): after ALL alignment -- the pass counts final alignments --, per (index, part), before the records are fetched
  uint64_t idc[4] = {0, 0, 0, 0};
  if (idcov) {
    for (size_t k = 0; k < dbs.size(); k++) {
      smr_params p = base;
      p.index_num = (uint32_t)k;
      for (size_t part = 0; part < dbs[k].parts.size(); part++) {
        p.part = (uint32_t)part;
        if (!keep_part && smr_index_upload(gpu, dbs[k].parts[part], 0) != SMR_OK) die(smr_last_error(gpu));
        for (size_t b = 0; b < rf.size(); b++)
          if (smr_batch_select(gpu, (int)b) != SMR_OK || smr_idcov_part(gpu, 0, &p, ro.min_id, ro.min_cov) != SMR_OK) die(smr_last_error(gpu));
        if (!keep_part) smr_index_unload(gpu, 0);
      }
    }
    for (size_t b = 0; b < rf.size(); b++) {
      uint64_t c4[4];
      if (smr_batch_select(gpu, (int)b) != SMR_OK || smr_idcov_counters(gpu, c4) != SMR_OK) die(smr_last_error(gpu));
      for (int q = 0; q < 4; q++) idc[q] += c4[q];
    }
  }
  for (size_t b = 0; b < rf.size(); b++) if (smr_batch_select(gpu, (int)b) != SMR_OK || smr_results_fetch(gpu) != SMR_OK) die(smr_last_error(gpu));

  // reports (writeReports, output.cpp:169-272)
  smr_report* rep = nullptr;
  std::string cmdline;
  for (int i = 0; i < argc; i++) { cmdline += argv[i]; cmdline += ' '; }       // the reference's opts.cmdline keeps the trailing blank
  uint64_t total_otu = 0;
  if (ro.fastx || ro.other || ro.blast_tabular || ro.blast_pairwise || ro.sam || idcov) {
    if (smr_report_open(out_dir.c_str(), &ro, is_fastq, &rep, err, sizeof err) != SMR_OK) die(err);
    if (ro.otu_map && smr_report_otu_count(rep, &total_otu) != SMR_OK) die("smr_report_otu_count failed");
    smr_report_set_cmdline(rep, cmdline.c_str());
    for (size_t k = 0; k < dbs.size(); k++) {
      smr_index_info info; smr_index_get_info(dbs[k].parts[0], &info);
      uint64_t fr = 0, fq = 0;
      smr_refstats_corrected(dbs[k].K, info.bg, info.full_len, info.numseq, n, total_len, &fr, &fq);
      smr_report_set_db(rep, (uint32_t)k, dbs[k].lambda, dbs[k].K, fr, fq);
      for (size_t part = 0; part < dbs[k].parts.size(); part++) smr_report_set_part(rep, (uint32_t)k, (uint32_t)part, dbs[k].parts[part]);
    }
  }
  // --split device: aligned.* / other.* of the whole input in one call (layout 0: single reads, 1: mates interleaved, 2: mates in batch 1); the
  // loop below then leaves those files alone, and needs the text of a read only for the BLAST and SAM rows
  const bool split_fx = split_device && rep && (ro.fastx || ro.other);
  if (split_fx) {
    smr_fxsplit_opts so; memset(&so, 0, sizeof so);
    so.layout = rf.size() == 2 ? 2 : paired ? 1 : 0;
    so.paired_in = ro.paired_in; so.paired_out = ro.paired_out; so.out2 = ro.out2; so.sout = ro.sout; so.want_aligned = ro.fastx; so.want_other = ro.other;
    uint64_t off[9], need = 0;
    if (smr_batch_select(gpu, 0) != SMR_OK || smr_fastx_split(gpu, so.layout == 2 ? 1 : -1, &so, nullptr, nullptr, 0, off, &need) != SMR_OK) die(smr_last_error(gpu));
    if (zip_device) {                                        // the streams are deflated where they are; only gzip members cross the bus
      uint64_t gz_off[9];
      std::vector<uint8_t> gz((size_t)smr_gzip_bound(need, need / smr_gzip_chunk() + 8) + 1);      // (at most one short chunk per stream)
      if (smr_fastx_split_gz(gpu, so.layout == 2 ? 1 : -1, &so, nullptr, gz.data(), gz.size(), gz_off, off, &need) != SMR_OK) die(smr_last_error(gpu));
      if (smr_report_add_fastx_gz(rep, gz.data(), gz_off) != SMR_OK) die(smr_report_last_error(rep));
    } else {
    std::vector<uint8_t> fx((size_t)need + 1);
    if (smr_fastx_split(gpu, so.layout == 2 ? 1 : -1, &so, nullptr, fx.data(), need, off, &need) != SMR_OK) die(smr_last_error(gpu));
    if (smr_report_add_fastx(rep, fx.data(), off) != SMR_OK) die(smr_report_last_error(rep));
    }
    smr_report_skip_fastx(rep, 1);
  }
  // --rows device: the SAM / BLAST rows of every (index, part) in one call each, after all alignment (the call order of smr_idcov_part); a run of
  // more than one part uploads each part again for it.  --pairwise device: the pairwise text of the part, while it is there
  // --otu device / --otu-mates device: the members of the map of the part from smr_otu_part / smr_otu_part_mates, in the same visit
  const bool map_dev = otu_dev && ro.otu_map;
  if (rows_dev || pair_dev || map_dev) {
    std::vector<uint8_t> rb;
    std::vector<smr_otu_group> gb;
    if (smr_batch_select(gpu, 0) != SMR_OK) die(smr_last_error(gpu));
    // --mates device: the same calls in their form for mates in two files (batch 0 selected, the mates in batch 1)
    auto rows_part = [&](const smr_params* p, const smr_index* ix, const smr_rows_opts* o, uint8_t* b, uint64_t cap, uint64_t* off, uint64_t* need) {
      return mates_device ? smr_rows_part_mates(gpu, 1, 0, p, ix, o, b, cap, off, need) : smr_rows_part(gpu, 0, p, ix, o, b, cap, off, need);
    };
    auto rows_part_gz = [&](const smr_params* p, const smr_index* ix, const smr_rows_opts* o, uint8_t* b, uint64_t cap, uint64_t* gz_off, uint64_t* off, uint64_t* need) {
      return mates_device ? smr_rows_part_mates_gz(gpu, 1, 0, p, ix, o, b, cap, gz_off, off, need) : smr_rows_part_gz(gpu, 0, p, ix, o, b, cap, gz_off, off, need);
    };
    auto pairwise_part = [&](const smr_params* p, const smr_index* ix, const smr_rows_opts& o, uint8_t* b, uint64_t cap, uint64_t* need) {
      return mates_device ? smr_pairwise_part_mates(gpu, 1, 0, p, ix, o.lambda, o.K, o.full_ref_corr, o.full_read_corr, b, cap, need)
                          : smr_pairwise_part(gpu, 0, p, ix, o.lambda, o.K, o.full_ref_corr, o.full_read_corr, b, cap, need);
    };
    auto otu_part = [&](const smr_params* p, const smr_index* ix, uint8_t* b, uint64_t cap, smr_otu_group* g, uint64_t gcap, uint64_t* need2, int* any) {
      return otu_mates_device ? smr_otu_part_mates(gpu, 1, 0, p, ix, ro.min_id, ro.min_cov, b, cap, g, gcap, need2, any)
                              : smr_otu_part(gpu, 0, p, ix, ro.min_id, ro.min_cov, b, cap, g, gcap, need2, any);
    };
    auto pairwise_part_gz = [&](const smr_params* p, const smr_index* ix, const smr_rows_opts& o, uint8_t* b, uint64_t cap, uint64_t* plain, uint64_t* need) {
      return mates_device ? smr_pairwise_part_mates_gz(gpu, 1, 0, p, ix, o.lambda, o.K, o.full_ref_corr, o.full_read_corr, b, cap, plain, need)
                          : smr_pairwise_part_gz(gpu, 0, p, ix, o.lambda, o.K, o.full_ref_corr, o.full_read_corr, b, cap, plain, need);
    };
    for (size_t k = 0; k < dbs.size(); k++) {
      smr_index_info info; smr_index_get_info(dbs[k].parts[0], &info);
      smr_params p = base;
      p.minimal_score = smr_minimal_score(dbs[k].lambda, dbs[k].K, info.bg, info.full_len, info.numseq, n, total_len, evalue);
      p.index_num = (uint32_t)k;
      smr_rows_opts wo; memset(&wo, 0, sizeof wo);
      wo.want_sam = ro.sam; wo.want_blast = ro.blast_tabular; memcpy(wo.blast_cols, ro.blast_cols, sizeof wo.blast_cols);
      wo.lambda = dbs[k].lambda; wo.K = dbs[k].K;
      smr_refstats_corrected(dbs[k].K, info.bg, info.full_len, info.numseq, n, total_len, &wo.full_ref_corr, &wo.full_read_corr);
      for (size_t part = 0; part < dbs[k].parts.size(); part++) {
        p.part = (uint32_t)part;
        if (!keep_part && smr_index_upload(gpu, dbs[k].parts[part], 0) != SMR_OK) die(smr_last_error(gpu));
        uint64_t off[3], need = 0;
        // --ziprows device: the buffer is sized once, by smr_gzip_lines_bound of what a sizes-only PLAIN call returns (two cheap kernels); a
        // sizes-only _gz call would run the matching, most of a compression, twice
        if (rows_dev && ziprows_device) {
          uint64_t gz_off[3];
          if (rows_part(&p, dbs[k].parts[part], &wo, nullptr, 0, off, &need) != SMR_OK) die(smr_last_error(gpu));
          const uint64_t bound = smr_gzip_lines_bound(need, 2);
          if (rb.size() < bound + 1) rb.resize((size_t)bound + 1);
          if (rows_part_gz(&p, dbs[k].parts[part], &wo, rb.data(), bound, gz_off, off, &need) != SMR_OK) die(smr_last_error(gpu));
          if (smr_report_add_rows_gz(rep, (uint32_t)k, (uint32_t)part, rb.data(), gz_off) != SMR_OK) die(smr_report_last_error(rep));
        } else if (rows_dev) {
          if (rows_part(&p, dbs[k].parts[part], &wo, nullptr, 0, off, &need) != SMR_OK) die(smr_last_error(gpu));
          if (rb.size() < need + 1) rb.resize((size_t)need + 1);
          if (need && rows_part(&p, dbs[k].parts[part], &wo, rb.data(), need, off, &need) != SMR_OK) die(smr_last_error(gpu));
          if (smr_report_add_rows(rep, (uint32_t)k, (uint32_t)part, rb.data(), off) != SMR_OK) die(smr_report_last_error(rep));
        }
        if (pair_dev && ziprows_device) {
          uint64_t plain = 0;
          if (pairwise_part(&p, dbs[k].parts[part], wo, nullptr, 0, &need) != SMR_OK) die(smr_last_error(gpu));
          const uint64_t bound = smr_gzip_lines_bound(need, 1);
          if (rb.size() < bound + 1) rb.resize((size_t)bound + 1);
          if (pairwise_part_gz(&p, dbs[k].parts[part], wo, rb.data(), bound, &plain, &need) != SMR_OK) die(smr_last_error(gpu));
          if (smr_report_add_pairwise_gz(rep, (uint32_t)k, (uint32_t)part, rb.data(), need) != SMR_OK) die(smr_report_last_error(rep));
        } else if (pair_dev) {
          if (pairwise_part(&p, dbs[k].parts[part], wo, nullptr, 0, &need) != SMR_OK) die(smr_last_error(gpu));
          if (rb.size() < need + 1) rb.resize((size_t)need + 1);
          if (need && pairwise_part(&p, dbs[k].parts[part], wo, rb.data(), need, &need) != SMR_OK) die(smr_last_error(gpu));
          if (smr_report_add_pairwise(rep, (uint32_t)k, (uint32_t)part, rb.data(), need) != SMR_OK) die(smr_report_last_error(rep));
        }
        if (map_dev) {
          uint64_t need2[2] = {0, 0}; int any = 0;
          if (otu_part(&p, dbs[k].parts[part], nullptr, 0, nullptr, 0, need2, &any) != SMR_OK) die(smr_last_error(gpu));
          if (rb.size() < need2[0] + 1) rb.resize((size_t)need2[0] + 1);
          if (gb.size() < need2[1] + 1) gb.resize((size_t)need2[1] + 1);
          if (need2[1] && otu_part(&p, dbs[k].parts[part], rb.data(), need2[0], gb.data(), need2[1], need2, &any) != SMR_OK) die(smr_last_error(gpu));
          if (smr_report_add_otu(rep, (uint32_t)k, (uint32_t)part, rb.data(), need2[0], gb.data(), need2[1], any) != SMR_OK) die(smr_report_last_error(rep));
        }
        smr_index_unload(gpu, 0);
      }
    }
    if (map_dev) smr_report_skip_otu(rep, 1);
    if (rows_dev) smr_report_skip_rows(rep, 1);
    if (pair_dev) smr_report_skip_pairwise(rep, 1);
  }
  // --otu device: aligned_denovo.* of the whole input in one call (layout 0: single reads, 1: mates interleaved; --otu-mates device: 2, mates in batch 1)
  const bool dn_dev = otu_dev && ro.denovo;
  if (dn_dev) {
    smr_fxsplit_opts so; memset(&so, 0, sizeof so);
    so.layout = otu_mates_device ? 2 : paired ? 1 : 0;
    const int dn_mates = otu_mates_device ? 1 : -1;
    so.paired_in = ro.paired_in; so.paired_out = ro.paired_out; so.out2 = ro.out2; so.sout = ro.sout;
    uint64_t off[5], need = 0;
    if (smr_batch_select(gpu, 0) != SMR_OK || smr_fastx_denovo(gpu, dn_mates, &so, nullptr, nullptr, 0, off, &need) != SMR_OK) die(smr_last_error(gpu));
    if (zip_device) {
      uint64_t gz_off[5];
      std::vector<uint8_t> gz((size_t)smr_gzip_bound(need, need / smr_gzip_chunk() + 4) + 1);
      if (smr_fastx_denovo_gz(gpu, dn_mates, &so, nullptr, gz.data(), gz.size(), gz_off, off, &need) != SMR_OK) die(smr_last_error(gpu));
      if (smr_report_add_denovo_gz(rep, gz.data(), gz_off) != SMR_OK) die(smr_report_last_error(rep));
    } else {
    std::vector<uint8_t> fx((size_t)need + 1);
    if (need && smr_fastx_denovo(gpu, dn_mates, &so, nullptr, fx.data(), need, off, &need) != SMR_OK) die(smr_last_error(gpu));
    if (smr_report_add_denovo(rep, fx.data(), off) != SMR_OK) die(smr_report_last_error(rep));
    }
    smr_report_skip_denovo(rep, 1);
  }
  // does the report take the reads one by one at all: for aligned.* / other.*, for rows / pairwise text, for the map or aligned_denovo.* that no
  // device call has brought
  const bool feed = rep && (!split_fx || ((ro.sam || ro.blast_tabular) && !rows_dev) || (ro.blast_pairwise && !pair_dev) || (ro.otu_map && !map_dev) ||
                            (ro.denovo && !dn_dev));
  // kvdb.put(read.id, read.toBinString()) (processor.cpp:150-155) -> records.bin ; Readstats -> summary.txt
  const std::string rp = out_dir + "/records.bin", sp = out_dir + "/summary.txt";
  FILE* f = fopen(rp.c_str(), "wb");
  if (!f) die("cannot write " + rp);
  uint64_t nrec = 0;
  fwrite(&nrec, 8, 1, f);
  struct Mate { std::vector<uint8_t> rec; std::vector<char> h, s, q; };
  auto load = [&](size_t b, uint32_t i, Mate& m) {                  // record + text of read i of batch b
    smr_batch_select(gpu, (int)b);
    const size_t len = smr_result_record(gpu, i, nullptr, 0);
    m.rec.resize(len);
    if (len) smr_result_record(gpu, i, m.rec.data(), len);
    if (feed) {
      size_t tl[3];
      smr_reads_record_text(rf[b], i, nullptr, 0, nullptr, 0, nullptr, 0, tl);
      m.h.resize(tl[0] + 1); m.s.resize(tl[1] + 1); m.q.resize(tl[2] + 1);
      smr_reads_record_text(rf[b], i, m.h.data(), m.h.size(), m.s.data(), m.s.size(), m.q.data(), m.q.size(), tl);
    }
    if (len) {
      const std::string key = std::to_string(b) + "_" + std::to_string(i);      // KVDB key: <reads file>_<read number>
      const uint64_t kl = key.size(), vl = len;
      fwrite(&kl, 8, 1, f); fwrite(key.data(), 1, kl, f); fwrite(&vl, 8, 1, f); fwrite(m.rec.data(), 1, vl, f);
      nrec++;
    }
  };
  Mate m1, m2;
  if (paired) {
    const uint32_t np = rf.size() == 2 ? smr_reads_count(rf[0]) : smr_reads_count(rf[0]) / 2;
    for (uint32_t i = 0; i < np; i++) {
      if (rf.size() == 2) { load(0, i, m1); load(1, i, m2); } else { load(0, 2 * i, m1); load(0, 2 * i + 1, m2); }
      if (feed && smr_report_add_pair(rep, m1.h.data(), m1.s.data(), is_fastq ? m1.q.data() : nullptr, m1.rec.data(), m1.rec.size(),
                                      m2.h.data(), m2.s.data(), is_fastq ? m2.q.data() : nullptr, m2.rec.data(), m2.rec.size()) != SMR_OK) die(smr_report_last_error(rep));
    }
  } else {
    for (uint32_t i = 0; i < smr_reads_count(rf[0]); i++) {
      load(0, i, m1);
      if (feed && smr_report_add(rep, m1.h.data(), m1.s.data(), is_fastq ? m1.q.data() : nullptr, m1.rec.data(), m1.rec.size()) != SMR_OK) die(smr_report_last_error(rep));
    }
  }
  std::vector<uint64_t> ctr(2 + dbs.size(), 0), cb(2 + dbs.size());
  for (size_t b = 0; b < rf.size(); b++) {
    smr_batch_select(gpu, (int)b);
    smr_counters(gpu, cb.data(), (uint32_t)dbs.size());
    for (size_t k = 0; k < ctr.size(); k++) ctr[k] += cb[k];
  }
  {  // readstats.store_to_db(kvdb) (processor.cpp:283-284): one more KVDB entry, key = hash of the read files' names
    const char* rfn[2] = {reads_paths[0].c_str(), reads_paths.size() > 1 ? reads_paths[1].c_str() : nullptr};
    char key[32];
    const uint64_t kl = smr_readstats_key(rfn, (uint32_t)reads_paths.size(), key, sizeof key);
    std::vector<uint8_t> rs(smr_readstats_record(n, total_len, min_len, max_len, ctr[0], ctr[1], ctr.data() + 2, (uint32_t)dbs.size(), nullptr, 0));
    smr_readstats_record(n, total_len, min_len, max_len, ctr[0], ctr[1], ctr.data() + 2, (uint32_t)dbs.size(), rs.data(), rs.size());
    const uint64_t vl = rs.size();
    fwrite(&kl, 8, 1, f); fwrite(key, 1, kl, f); fwrite(&vl, 8, 1, f); fwrite(rs.data(), 1, vl, f);
    nrec++;
  }
  fseek(f, 0, SEEK_SET); fwrite(&nrec, 8, 1, f); fclose(f);
  if (rep && smr_report_close(rep) != SMR_OK) die("cannot write the report files");
  f = fopen(sp.c_str(), "w");
  if (!f) die("cannot write " + sp);
  fprintf(f, "Total reads = %llu\nTotal reads passing E-value threshold = %llu\nToo short reads (last part) = %llu\n", (unsigned long long)n,
          (unsigned long long)ctr[0], (unsigned long long)ctr[1]);
  for (size_t k = 0; k < dbs.size(); k++) fprintf(f, "%s\t%llu\n", dbs[k].fasta.c_str(), (unsigned long long)ctr[2 + k]);
  if (idcov) fprintf(f, "num_yid_ycov = %llu\nnum_yid_ncov = %llu\nnum_nid_ycov = %llu\nnum_denovo = %llu\nTotal OTUs = %llu\n", (unsigned long long)idc[0],
                     (unsigned long long)idc[1], (unsigned long long)idc[2], (unsigned long long)idc[3], (unsigned long long)total_otu);
  fclose(f);
  {  // aligned.log (Summary::write, summary.cpp:57-100)
    std::vector<smr_summary_db> sdb(dbs.size());
    for (size_t k = 0; k < dbs.size(); k++) {
      smr_index_info info; smr_index_get_info(dbs[k].parts[0], &info);
      sdb[k].ref_file = dbs[k].fasta.c_str();
      sdb[k].skiplengths[0] = info.lnwin; sdb[k].skiplengths[1] = info.lnwin / 2; sdb[k].skiplengths[2] = 3;
      sdb[k].lambda = dbs[k].lambda; sdb[k].K = dbs[k].K;
      sdb[k].minimal_score = smr_minimal_score(dbs[k].lambda, dbs[k].K, info.bg, info.full_len, info.numseq, n, total_len, evalue);
      sdb[k].reads_matched = ctr[2 + k];
    }
    const time_t now = time(nullptr);
    const std::string stamp = ctime(&now);
    const char* rfn[2] = {reads_paths[0].c_str(), reads_paths.size() > 1 ? reads_paths[1].c_str() : nullptr};
    smr_summary sm; memset(&sm, 0, sizeof sm);
    sm.cmdline = cmdline.c_str(); sm.pid = ""; sm.timestamp = stamp.c_str();
    sm.seed_len = 18; sm.num_seeds = base.num_seeds; sm.edges = base.edges; sm.match = base.match; sm.mismatch = base.mismatch;
    sm.gap_open = base.gap_open; sm.gap_ext = base.gap_ext; sm.score_N = base.score_N; sm.sam_sq = ro.sam_sq; sm.threads = 1;
    sm.reads_files = rfn; sm.n_reads_files = (uint32_t)reads_paths.size();
    sm.total_reads = n; sm.num_aligned = ctr[0]; sm.all_reads_len = total_len;
    sm.min_read_len = min_len; sm.max_read_len = max_len;
    sm.dbs = sdb.data(); sm.n_dbs = (uint32_t)sdb.size();
    sm.is_denovo = ro.denovo; sm.total_denovo = idc[3]; sm.is_otu_map = ro.otu_map; sm.total_id_cov = idc[0]; sm.total_otu = total_otu;
    if (smr_summary_write((out_dir + "/aligned.log").c_str(), &sm) != SMR_OK) die("cannot write aligned.log");
  }
  printf("%llu reads, %llu aligned, %llu records -> %s\n", (unsigned long long)n, (unsigned long long)ctr[0], (unsigned long long)nrec, rp.c_str());
  for (auto& d : dbs) for (auto* ix : d.parts) smr_index_free(ix);
  for (auto* r : rf) smr_reads_free(r);
  smr_destroy(gpu);
  return 0;
}
