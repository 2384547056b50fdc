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
typedef unsigned long long ull;
[[noreturn]] void die(const std::string& m) { fprintf(stderr, "ERROR: %s\n", m.c_str()); exit(EXIT_FAILURE); }

struct Db {
  std::string fasta, idx_prefix; double lambda = 0, K = 0; bool has_gumbel = false; std::vector<smr_index*> parts;
  // what load_indexes works out once, from the DB's statistics and the totals of the reads: the score a read needs to count as aligned and
  // the length-corrected sizes behind the e-values of the reports
  smr_index_info info; uint32_t minimal_score = 0; uint64_t full_ref_corr = 0, full_read_corr = 0;
};

struct Options {
  std::vector<Db> dbs;
  std::vector<std::string> reads_paths; std::string out_dir = ".", cmdline;
  int zip_out = -1;                                         // -1: like the reads file (options.hpp zip_out, report_fx_base.cpp:94)
  smr_params base; double evalue = 1.0; int device = 0;
  bool pack_device = false, split_device = false, rows_device = false, pair_device = false, otu_device = false, otu_mates_device = false, zip_device = false, unzip_device = false, ziprows_device = false, mates_device = false;
  bool id_given = false, cov_given = false;
  smr_report_opts ro;
  Options() { smr_params_default(&base); memset(&ro, 0, sizeof ro); }
  // what the switches come to, given the reports the run writes
  bool idcov() const { return ro.otu_map || ro.denovo; }
  bool report() const { return ro.fastx || ro.other || ro.blast_tabular || ro.blast_pairwise || ro.sam || idcov(); }
  bool split_fx() const { return split_device && report() && (ro.fastx || ro.other); }
  bool rows_dev() const { return rows_device && (ro.sam || ro.blast_tabular); }
  bool pair_dev() const { return pair_device && !ro.blast_tabular; }            // (with tabular rows as well the host writes no pairwise text either)
  bool otu_dev() const { return (otu_device || otu_mates_device) && idcov(); }  // (two reads files: --otu-mates device, the calls in their form for mates)
  bool map_dev() const { return otu_dev() && ro.otu_map; }
  bool dn_dev() const { return otu_dev() && ro.denovo; }
  // does the report take the reads one by one at all: for aligned.* / other.*, for rows / pairwise text, for the map or aligned_denovo.* that no
  // device call has brought
  bool feed() const {
    return report() && (!split_fx() || ((ro.sam || ro.blast_tabular) && !rows_dev()) || (ro.blast_pairwise && !pair_dev()) || (ro.otu_map && !map_dev()) ||
                        (ro.denovo && !dn_dev()));
  }
};

// the context, the batches (one per reads file) and what is known of the reads once they are loaded
struct Run {
  smr_ctx* gpu = nullptr; std::vector<smr_reads*> rf; uint32_t slots = 0;
  uint64_t n = 0, total_len = 0; uint32_t min_len = 0xFFFFFFFFu, max_len = 0; bool is_fastq = false, paired = false;
};

// the switches that take host | device, as -name or --name
const struct { const char* name; bool Options::*on; } kSwitches[] = {
    {"pack", &Options::pack_device}, {"split", &Options::split_device}, {"rows", &Options::rows_device}, {"pairwise", &Options::pair_device},
    {"unzip", &Options::unzip_device}, {"zip", &Options::zip_device}, {"ziprows", &Options::ziprows_device}, {"mates", &Options::mates_device},
    {"otu-mates", &Options::otu_mates_device}, {"otu", &Options::otu_device}};
// the options without a value that ask for a report or say how it is laid out
const struct { const char* name; int smr_report_opts::*on; } kReportFlags[] = {
    {"otu_map", &smr_report_opts::otu_map}, {"de_novo_otu", &smr_report_opts::denovo}, {"fastx", &smr_report_opts::fastx}, {"other", &smr_report_opts::other},
    {"sam", &smr_report_opts::sam}, {"SQ", &smr_report_opts::sam_sq}, {"paired_in", &smr_report_opts::paired_in}, {"paired_out", &smr_report_opts::paired_out},
    {"out2", &smr_report_opts::out2}, {"sout", &smr_report_opts::sout}};
// the row of such a table that `a` names, or the table's end
template <class Row, size_t N> const Row* find_option(const Row (&table)[N], const std::string& a) {
  const Row* row = table;
  while (row != table + N && a != std::string("-") + row->name && a != std::string("--") + row->name) row++;
  return row;
}

Options parse_options(int argc, char** argv) {
  Options o; std::vector<Db>& dbs = o.dbs; smr_params& base = o.base; smr_report_opts& ro = o.ro;
  for (int i = 0; i < argc; i++) { o.cmdline += argv[i]; o.cmdline += ' '; }   // the reference's opts.cmdline keeps the trailing blank
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    auto val = [&]() -> std::string { if (i + 1 >= argc) die("missing value after " + a); return argv[++i]; };
    const auto* sw = find_option(kSwitches, a);
    const auto* flag = find_option(kReportFlags, a);
    if (sw != std::end(kSwitches)) { const std::string v = val(); if (v != "host" && v != "device") die(std::string("--") + sw->name + ": host or device"); o.*sw->on = v == "device"; }
    else if (a == "-ref" || a == "--ref") { Db d; d.fasta = val(); dbs.push_back(d); }
    else if (a == "-idx" || a == "--idx") { if (dbs.empty()) die("--idx before --ref"); dbs.back().idx_prefix = val(); }   // reference-format index files
    else if (a == "-gumbel" || a == "--gumbel") { if (dbs.empty()) die("--gumbel before --ref"); dbs.back().lambda = atof(val().c_str()); dbs.back().K = atof(val().c_str()); dbs.back().has_gumbel = true; }
    else if (a == "-reads" || a == "--reads") { if (o.reads_paths.size() == 2) die("at most two --reads files (mates)"); o.reads_paths.push_back(val()); }
    else if (a == "-out" || a == "--out") o.out_dir = val();
    else if (a == "-e") o.evalue = atof(val().c_str());
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
    else if (a == "-device") o.device = atoi(val().c_str());
    else if (flag != std::end(kReportFlags)) ro.*flag->on = 1;
    else if (a == "-id" || a == "--id") { ro.min_id = atof(val().c_str()); o.id_given = true; }
    else if (a == "-coverage" || a == "--coverage") { ro.min_cov = atof(val().c_str()); o.cov_given = true; }
    else if (a == "-zip-out" || a == "--zip-out") { const std::string v = val(); o.zip_out = (v == "1" || v == "true" || v == "t" || v == "yes" || v == "y") ? 1 : 0; }
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
      exit(0);
    } else die("unknown option " + a);
  }
  return o;
}

// every refusal that needs no file, in a fixed order; nothing is loaded or written before the last has passed.  Settles the defaults of -id /
// -coverage and whether the reports are gzipped
void check_options(Options& o) {
  smr_report_opts& ro = o.ro;
  const size_t n_files = o.reads_paths.size();
  if (o.mates_device && n_files < 2) die("--mates device interleaves the rows of mates in two reads files on the device: it needs two --reads files");
  if (o.mates_device && !o.rows_device && !o.pair_device) die("--mates device interleaves what --rows device and --pairwise device write for two reads files: it needs one of the two");
  if (o.split_device && !o.pack_device) die("--split device writes aligned.* / other.* from the text the device parsed: it needs --pack device");
  if (o.unzip_device && !o.pack_device) die("--unzip device inflates a gzip reads file into the text buffer the device parses: it needs --pack device");
  if (o.rows_device && !o.pack_device) die("--rows device writes the SAM / BLAST rows from the text the device parsed: it needs --pack device");
  if (o.pair_device && !o.pack_device) die("--pairwise device writes the BLAST pairwise text from the text the device parsed: it needs --pack device");
  if (o.pair_device && !ro.blast_pairwise) die("--pairwise device writes the pairwise text of --blast 0: without --blast 0 there is none");
  if (o.pair_device && n_files == 2 && !o.mates_device) die("--pairwise device takes one reads file (single reads or interleaved mates): the blocks of mates in two files alternate between the batches and stay with --pairwise host");
  if (o.rows_device && ro.blast_pairwise && !o.pair_device) die("--rows device writes BLAST tabular rows only: --blast 0 (pairwise) stays with --rows host");
  if (o.rows_device && n_files == 2 && !o.mates_device) die("--rows device takes one reads file (single reads or interleaved mates): the rows of mates in two files alternate between the batches and stay with --rows host");
  // the reference's rules for the four options (options.cpp:1623-1628, 1667-1674, 1744-1757)
  if ((o.id_given || o.cov_given) && !ro.otu_map) die("options '-id' and '-coverage' can only be used together with '-otu_map': they are the thresholds of the OTU map");
  if (ro.otu_map && !o.base.is_best) die("option '-otu_map' cannot be used with '-no-best': the OTU map is built from the best alignments");
  if (ro.otu_map) { if (!o.id_given) ro.min_id = 0.97; if (!o.cov_given) ro.min_cov = 0.97; }
  if (!(ro.min_id >= 0 && ro.min_id <= 1 && ro.min_cov >= 0 && ro.min_cov <= 1)) die("-id and -coverage take a value within [0, 1]");
  if (o.otu_device && !o.pack_device) die("--otu device writes the OTU map and aligned_denovo.* from the text the device parsed: it needs --pack device");
  if (o.otu_device && n_files == 2) die("--otu device takes one reads file (single reads or interleaved mates): the members of a group of mates in two files alternate between the batches and stay with --otu host");
  if (o.otu_mates_device && n_files < 2) die("--otu-mates device writes the OTU map and aligned_denovo.* of mates in two reads files on the device: it needs two --reads files");
  if (o.otu_mates_device && !o.pack_device) die("--otu-mates device writes the OTU map and aligned_denovo.* from the text the device parsed: it needs --pack device");
  if (o.dbs.empty() || n_files == 0) die("--ref and --reads are required (see --help)");
  if (const char* why = smr_params_refused(&o.base)) die(std::string("these options are outside what libsmr_hip aligns (the reference accepts them): ") + why);
  // minimal_score (which reads count as aligned) and the e-values / bit scores of the BLAST report depend on the Gumbel parameters of the
  // (scoring scheme, DB background) pair.  The reference computes them per DB with its vendored NCBI ALP library (refstats.cpp:194-233),
  // which is outside this library: they must be given -- from the reference's log ("Gumbel lambda = ..", "Gumbel K = ..") for the same DB
  // and the same -match/-mismatch/-gap_open/-gap_ext.  No default is assumed: a silent guess would classify a different set of reads.
  for (auto& d : o.dbs) if (!d.has_gumbel) die("--gumbel LAMBDA K is required after every --ref (see --help): the values of the reference's log for this DB and scoring scheme");
  if (o.zip_out == -1) {                                    // gzip reports for a gzip reads file
    unsigned char mg[2] = {0, 0};
    if (FILE* fz = fopen(o.reads_paths[0].c_str(), "rb")) { if (fread(mg, 1, 2, fz) != 2) mg[0] = 0; fclose(fz); }
    o.zip_out = (mg[0] == 0x1f && mg[1] == 0x8b) ? 1 : 0;
  }
  ro.zip_out = o.zip_out;
  if (o.zip_device && !o.split_device) die("--zip device compresses the aligned.* / other.* streams where --split device leaves them: it needs --split device");
  if (o.zip_device && !o.zip_out) die("--zip device writes gzip members: the reports of this run are not gzipped (a plain reads file without -zip-out 1, or -zip-out 0)");
  if (o.ziprows_device && !o.rows_device && !o.pair_device) die("--ziprows device compresses the SAM / BLAST rows and the pairwise text where --rows device and --pairwise device leave them: it needs one of the two");
  if (o.ziprows_device && !o.zip_out) die("--ziprows device writes gzip members: the reports of this run are not gzipped (a plain reads file without -zip-out 1, or -zip-out 0)");
}

// reads (Readfeed::next -> Read::init, readfeed.hpp:124 / read.cpp:264-347)
// (all cores parse and 2-bit pack the FASTA / FASTQ / .gz file; the text stays mapped for the report writers)
// one batch per reads file (the second file holds the mates of the first: options.cpp:1591 is_paired)
// (--pack device: the kernels of the engine do that, straight into batch b; what comes back has the text, the record offsets and the lengths)
void load_reads(const Options& o, Run& r) {
  char err[512] = "";
  r.rf.assign(o.reads_paths.size(), nullptr);
  r.slots = o.base.num_alignments > 0 ? o.base.num_alignments : 256;
  const uint32_t flags = SMR_FASTX_VIEW | (o.unzip_device ? SMR_FASTX_INFLATE : 0u) | ((o.split_device || o.rows_device || o.pair_device || o.otu_dev()) ? SMR_FASTX_KEEP : 0u);
  if (o.pack_device && smr_create(o.device, &r.gpu, err, sizeof err) != SMR_OK) die(err);
  for (size_t b = 0; b < r.rf.size(); b++) {
    if (o.pack_device) {
      if (smr_batch_select(r.gpu, (int)b) != SMR_OK) die(smr_last_error(r.gpu));
      if (smr_reads_upload_fastx_file(r.gpu, o.reads_paths[b].c_str(), r.slots, flags, &r.rf[b], err, sizeof err) != SMR_OK) die(err);
    } else if (smr_reads_load_fastx_text(o.reads_paths[b].c_str(), 0, &r.rf[b], err, sizeof err) != SMR_OK) die(err);
    r.n += smr_reads_count(r.rf[b]); r.total_len += smr_reads_total_len(r.rf[b]);
    if (smr_reads_count(r.rf[b])) { r.min_len = std::min(r.min_len, smr_reads_min_len(r.rf[b])); r.max_len = std::max(r.max_len, smr_reads_max_len(r.rf[b])); }
  }
  if (r.n == 0) r.min_len = 0;
  r.is_fastq = smr_reads_is_fastq(r.rf[0]) != 0;
  r.paired = r.rf.size() == 2 || o.ro.paired_in || o.ro.paired_out;
  if (r.rf.size() == 2 && smr_reads_count(r.rf[0]) != smr_reads_count(r.rf[1])) die("the two --reads files hold different numbers of reads");
  if (r.rf.size() == 1 && r.paired && (smr_reads_count(r.rf[0]) & 1)) die("-paired_in / -paired_out with one file: odd number of reads");
}

// indexes: reference-built files when a prefix is given, else our own builder (Index ctor / build_index, index.cpp:61-107); then, per DB, the
// values that depend on it and on the totals of the reads (Refstats)
void load_indexes(const Run& r, double evalue, std::vector<Db>& dbs) {
  char err[512] = "";
  for (auto& d : dbs) {
    const bool files = !d.idx_prefix.empty();
    if (files) {
      smr_index* p0 = nullptr;
      if (smr_index_load_files(d.idx_prefix.c_str(), 0, d.fasta.c_str(), &p0, err, sizeof err) != SMR_OK) die(err);
      d.parts.push_back(p0);
    } else {
      smr_index* arr[256]; uint32_t np = 0;
      if (smr_index_build(d.fasta.c_str(), 18, 3072.0, 10000, 0, arr, 256, &np, err, sizeof err) != SMR_OK) die(err);
      d.parts.assign(arr, arr + np);
    }
    smr_index_get_info(d.parts[0], &d.info);
    for (uint32_t k = 1; files && k < d.info.n_parts; k++) {
      smr_index* pk = nullptr;
      if (smr_index_load_files(d.idx_prefix.c_str(), k, d.fasta.c_str(), &pk, err, sizeof err) != SMR_OK) die(err);
      d.parts.push_back(pk);
    }
    d.minimal_score = smr_minimal_score(d.lambda, d.K, d.info.bg, d.info.full_len, d.info.numseq, r.n, r.total_len, evalue);
    smr_refstats_corrected(d.K, d.info.bg, d.info.full_len, d.info.numseq, r.n, r.total_len, &d.full_ref_corr, &d.full_read_corr);
  }
}

// the context, unless --pack device has made it, and the batches --pack host has parsed
void upload_reads(const Options& o, Run& r) {
  char err[512] = "";
  if (!r.gpu && smr_create(o.device, &r.gpu, err, sizeof err) != SMR_OK) die(err);
  if (smr_sw_mode(r.gpu, -1) == 0) fprintf(stderr, "smr_align: the 32-bit Smith-Waterman kernel is in use (packed kernel off or failed its self-check): expect about half the alignment rate\n");
  for (size_t b = 0; !o.pack_device && b < r.rf.size(); b++)
    if (smr_batch_select(r.gpu, (int)b) != SMR_OK || smr_reads_upload(r.gpu, r.rf[b], r.slots) != SMR_OK) die(smr_last_error(r.gpu));
}

// The (index, part) loop of processor.cpp:219-277: visit(db, p) for every part in --ref order, p = base with index_num and part set (and what an
// earlier visit of the same index left in it).  upload: the part goes to slot 0 first; unload: slot 0 is emptied afterwards
template <class Visit> void for_each_part(smr_ctx* gpu, const smr_params& base, const std::vector<Db>& dbs, bool upload, bool unload, Visit visit) {
  for (size_t k = 0; k < dbs.size(); k++) {
    smr_params p = base;
    p.index_num = (uint32_t)k;
    for (size_t part = 0; part < dbs[k].parts.size(); part++) {
      p.part = (uint32_t)part;
      if (upload && smr_index_upload(gpu, dbs[k].parts[part], 0) != SMR_OK) die(smr_last_error(gpu));
      visit(dbs[k], p);
      if (unload) smr_index_unload(gpu, 0);
    }
  }
}

void align_parts(const Run& r, const Options& o, const std::vector<Db>& dbs, bool keep_part) {
  for_each_part(r.gpu, o.base, dbs, true, !keep_part, [&](const Db& db, smr_params& p) {
    p.minimal_score = db.minimal_score;
    p.is_last_index_part = (&db == &dbs.back() && p.part + 1 == db.parts.size());
    for (size_t b = 0; b < r.rf.size(); b++)
      if (smr_batch_select(r.gpu, (int)b) != SMR_OK || smr_align_part(r.gpu, 0, &p) != SMR_OK || smr_traceback(r.gpu, 0, &p) != SMR_OK) die(smr_last_error(r.gpu));
  });
}

// denovo_stats (processor.cpp:287-438): after ALL alignment -- the pass counts final alignments --, per (index, part), before the records are fetched
void idcov_parts(const Run& r, const Options& o, const std::vector<Db>& dbs, bool keep_part, uint64_t idc[4]) {
  for_each_part(r.gpu, o.base, dbs, !keep_part, !keep_part, [&](const Db&, smr_params& p) {
    for (size_t b = 0; b < r.rf.size(); b++)
      if (smr_batch_select(r.gpu, (int)b) != SMR_OK || smr_idcov_part(r.gpu, 0, &p, o.ro.min_id, o.ro.min_cov) != SMR_OK) die(smr_last_error(r.gpu));
  });
  for (size_t b = 0; b < r.rf.size(); b++) {
    uint64_t c4[4];
    if (smr_batch_select(r.gpu, (int)b) != SMR_OK || smr_idcov_counters(r.gpu, c4) != SMR_OK) die(smr_last_error(r.gpu));
    for (int q = 0; q < 4; q++) idc[q] += c4[q];
  }
}

// reports (writeReports, output.cpp:169-272)
smr_report* open_report(const Run& r, const Options& o, const std::vector<Db>& dbs, uint64_t* total_otu) {
  char err[512] = "";
  smr_report* rep = nullptr;
  if (smr_report_open(o.out_dir.c_str(), &o.ro, r.is_fastq, &rep, err, sizeof err) != SMR_OK) die(err);
  if (o.ro.otu_map && smr_report_otu_count(rep, total_otu) != SMR_OK) die("smr_report_otu_count failed");
  smr_report_set_cmdline(rep, o.cmdline.c_str());
  for (size_t k = 0; k < dbs.size(); k++) {
    smr_report_set_db(rep, (uint32_t)k, dbs[k].lambda, dbs[k].K, dbs[k].full_ref_corr, dbs[k].full_read_corr);
    for (size_t part = 0; part < dbs[k].parts.size(); part++) smr_report_set_part(rep, (uint32_t)k, (uint32_t)part, dbs[k].parts[part]);
  }
  return rep;
}

// The size-then-fill protocol of smr_hip.h.  call(nullptr, 0) asks for the sizes only and leaves in `need` whether there is anything to fetch;
// buf grows to cap_of(need) + 1 bytes and call(buf.data(), cap_of(need)) fills it -- unless need is 0 and `always` is not set.  A gz form hands
// its plain twin the sizes-only call, a gzip bound as cap_of, and sets `always`: that one filling call is its only call.
template <class CapOf, class Call> void size_then_fill(smr_ctx* gpu, std::vector<uint8_t>& buf, const uint64_t& need, bool always, CapOf cap_of, Call call) {
  if (call(nullptr, 0) != SMR_OK) die(smr_last_error(gpu));
  const uint64_t cap = cap_of(need);
  if (buf.size() < cap + 1) buf.resize((size_t)cap + 1);
  if ((always || need) && call(buf.data(), cap) != SMR_OK) die(smr_last_error(gpu));
}
uint64_t as_needed(uint64_t need) { return need; }
// the FASTX streams are deflated where they are and only gzip members cross the bus: at most one short chunk per stream
uint64_t fastx_gz_cap(uint64_t need, uint64_t streams) { return smr_gzip_bound(need, need / smr_gzip_chunk() + streams) + 1; }

// layout 0: single reads, 1: mates interleaved, 2: mates in batch 1; streams: want_aligned / want_other from --fastx / --other (the split's)
smr_fxsplit_opts fx_opts(const smr_report_opts& ro, int layout, bool streams) {
  smr_fxsplit_opts so; memset(&so, 0, sizeof so);
  if (streams) { so.want_aligned = ro.fastx; so.want_other = ro.other; }
  so.layout = layout; so.paired_in = ro.paired_in; so.paired_out = ro.paired_out; so.out2 = ro.out2; so.sout = ro.sout;
  return so;
}

// The FASTX streams of the whole input in one call, instead of read by read.  --split device: aligned.* / other.*; the per-read loop then leaves
// those files alone, and needs the text of a read only for the BLAST and SAM rows.  --otu device / --otu-mates device: aligned_denovo.*
struct FastxWriter {
  decltype(&smr_fastx_split) plain; decltype(&smr_fastx_split_gz) gz; decltype(&smr_report_add_fastx) add; decltype(&smr_report_add_fastx_gz) add_gz;
  decltype(&smr_report_skip_fastx) skip; uint64_t streams; bool fill_empty;
};
const FastxWriter kSplit = {smr_fastx_split, smr_fastx_split_gz, smr_report_add_fastx, smr_report_add_fastx_gz, smr_report_skip_fastx, 8, true};
const FastxWriter kDenovo = {smr_fastx_denovo, smr_fastx_denovo_gz, smr_report_add_denovo, smr_report_add_denovo_gz, smr_report_skip_denovo, 4, false};

void fastx_stage(const Run& r, const Options& o, smr_report* rep, const FastxWriter& w, const smr_fxsplit_opts& so) {
  smr_ctx* gpu = r.gpu;
  const int mates = so.layout == 2 ? 1 : -1;
  uint64_t off[9], gz_off[9], need = 0;
  std::vector<uint8_t> fx;
  const auto plain = [&](uint8_t* b, uint64_t cap) { return w.plain(gpu, mates, &so, nullptr, b, cap, off, &need); };
  if (smr_batch_select(gpu, 0) != SMR_OK) die(smr_last_error(gpu));
  if (o.zip_device) {
    size_then_fill(gpu, fx, need, true, [&](uint64_t n) { return fastx_gz_cap(n, w.streams); },
                   [&](uint8_t* b, uint64_t cap) { return b ? w.gz(gpu, mates, &so, nullptr, b, cap, gz_off, off, &need) : plain(nullptr, 0); });
    if (w.add_gz(rep, fx.data(), gz_off) != SMR_OK) die(smr_report_last_error(rep));
  } else {
    size_then_fill(gpu, fx, need, w.fill_empty, as_needed, plain);
    if (w.add(rep, fx.data(), off) != SMR_OK) die(smr_report_last_error(rep));
  }
  w.skip(rep, 1);
}

// The device writers of one (index, part) under the signatures of the plain calls.  --mates device (rows, pairwise text) and --otu-mates device
// (the map) put the form for mates in two files there: batch 0 selected, the mates in batch 1
template <auto Mates, class... A> int with_mates(smr_ctx* c, int slot, A... a) { return Mates(c, 1, slot, a...); }
struct PartWriters {
  decltype(&smr_rows_part) rows = smr_rows_part; decltype(&smr_rows_part_gz) rows_gz = smr_rows_part_gz;
  decltype(&smr_pairwise_part) pairwise = smr_pairwise_part; decltype(&smr_pairwise_part_gz) pairwise_gz = smr_pairwise_part_gz;
  decltype(&smr_otu_part) otu = smr_otu_part;
  explicit PartWriters(const Options& o) {
    if (o.mates_device) { rows = with_mates<smr_rows_part_mates>; rows_gz = with_mates<smr_rows_part_mates_gz>; pairwise = with_mates<smr_pairwise_part_mates>; pairwise_gz = with_mates<smr_pairwise_part_mates_gz>; }
    if (o.otu_mates_device) otu = with_mates<smr_otu_part_mates>;
  }
};

// what the device writes of one resident (index, part): SAM / BLAST rows, pairwise text, the members of the map.  rb, gb: buffers kept between parts
void visit_part(const Run& r, const Options& o, const Db& db, const smr_params& p, smr_report* rep, const PartWriters& w, std::vector<uint8_t>& rb, std::vector<smr_otu_group>& gb) {
  smr_ctx* gpu = r.gpu; const smr_index* ix = db.parts[p.part]; const uint32_t k = p.index_num, part = p.part;
  smr_rows_opts wo; memset(&wo, 0, sizeof wo);
  wo.want_sam = o.ro.sam; wo.want_blast = o.ro.blast_tabular; memcpy(wo.blast_cols, o.ro.blast_cols, sizeof wo.blast_cols);
  wo.lambda = db.lambda; wo.K = db.K; wo.full_ref_corr = db.full_ref_corr; wo.full_read_corr = db.full_read_corr;
  uint64_t off[3], gz_off[3], need = 0, plain = 0;
  const auto rows = [&](uint8_t* b, uint64_t cap) { return w.rows(gpu, 0, &p, ix, &wo, b, cap, off, &need); };
  const auto pairwise = [&](uint8_t* b, uint64_t cap) { return w.pairwise(gpu, 0, &p, ix, wo.lambda, wo.K, wo.full_ref_corr, wo.full_read_corr, b, cap, &need); };
  // --ziprows device: the buffer is sized once, by smr_gzip_lines_bound of what a sizes-only PLAIN call returns (two cheap kernels); a
  // sizes-only _gz call would run the matching, most of a compression, twice
  if (o.rows_dev() && o.ziprows_device) {
    size_then_fill(gpu, rb, need, true, [](uint64_t n) { return smr_gzip_lines_bound(n, 2); },
                   [&](uint8_t* b, uint64_t cap) { return b ? w.rows_gz(gpu, 0, &p, ix, &wo, b, cap, gz_off, off, &need) : rows(nullptr, 0); });
    if (smr_report_add_rows_gz(rep, k, part, rb.data(), gz_off) != SMR_OK) die(smr_report_last_error(rep));
  } else if (o.rows_dev()) {
    size_then_fill(gpu, rb, need, false, as_needed, rows);
    if (smr_report_add_rows(rep, k, part, rb.data(), off) != SMR_OK) die(smr_report_last_error(rep));
  }
  if (o.pair_dev() && o.ziprows_device) {
    size_then_fill(gpu, rb, need, true, [](uint64_t n) { return smr_gzip_lines_bound(n, 1); }, [&](uint8_t* b, uint64_t cap) {
      return b ? w.pairwise_gz(gpu, 0, &p, ix, wo.lambda, wo.K, wo.full_ref_corr, wo.full_read_corr, b, cap, &plain, &need) : pairwise(nullptr, 0); });
    if (smr_report_add_pairwise_gz(rep, k, part, rb.data(), need) != SMR_OK) die(smr_report_last_error(rep));
  } else if (o.pair_dev()) {
    size_then_fill(gpu, rb, need, false, as_needed, pairwise);
    if (smr_report_add_pairwise(rep, k, part, rb.data(), need) != SMR_OK) die(smr_report_last_error(rep));
  }
  if (o.map_dev()) {             // two buffers: need2 = {bytes, groups}; the groups decide whether there is anything to fetch
    uint64_t need2[2] = {0, 0}; int any = 0;
    size_then_fill(gpu, rb, need2[1], false, [&](uint64_t) { return need2[0]; }, [&](uint8_t* b, uint64_t cap) {
      if (b && gb.size() < need2[1] + 1) gb.resize((size_t)need2[1] + 1);
      return w.otu(gpu, 0, &p, ix, o.ro.min_id, o.ro.min_cov, b, cap, b ? gb.data() : nullptr, b ? need2[1] : 0, need2, &any); });
    if (smr_report_add_otu(rep, k, part, rb.data(), need2[0], gb.data(), need2[1], any) != SMR_OK) die(smr_report_last_error(rep));
  }
}

// --rows device: the SAM / BLAST rows of every (index, part) in one call each, after all alignment (the call order of smr_idcov_part); a run of
// more than one part uploads each part again for it.  --pairwise device: the pairwise text of the part, while it is there
// --otu device / --otu-mates device: the members of the map of the part from smr_otu_part / smr_otu_part_mates, in the same visit
void visit_parts(const Run& r, const Options& o, const std::vector<Db>& dbs, bool keep_part, smr_report* rep) {
  std::vector<uint8_t> rb;
  std::vector<smr_otu_group> gb(1);
  const PartWriters w(o);
  if (smr_batch_select(r.gpu, 0) != SMR_OK) die(smr_last_error(r.gpu));
  for_each_part(r.gpu, o.base, dbs, !keep_part, true, [&](const Db& db, smr_params& p) {
    p.minimal_score = db.minimal_score;
    visit_part(r, o, db, p, rep, w, rb, gb);
  });
  if (o.map_dev()) smr_report_skip_otu(rep, 1);
  if (o.rows_dev()) smr_report_skip_rows(rep, 1);
  if (o.pair_dev()) smr_report_skip_pairwise(rep, 1);
}

// kvdb.put(read.id, read.toBinString()) (processor.cpp:150-155) -> records.bin, the reads fed to the report on the way; ctr: the counters of all
// batches (num_aligned, num_short, reads matched per DB); -> the number of records
uint64_t write_records(const Run& r, const Options& o, size_t n_dbs, smr_report* rep, std::vector<uint64_t>& ctr) {
  const std::string rp = o.out_dir + "/records.bin";
  const bool feed = o.feed(), is_fastq = r.is_fastq;
  FILE* f = fopen(rp.c_str(), "wb");
  if (!f) die("cannot write " + rp);
  uint64_t nrec = 0;
  fwrite(&nrec, 8, 1, f);
  const auto put = [&](const void* key, uint64_t kl, const void* v, uint64_t vl) { fwrite(&kl, 8, 1, f); fwrite(key, 1, kl, f); fwrite(&vl, 8, 1, f); fwrite(v, 1, vl, f); nrec++; };
  struct Mate { std::vector<uint8_t> rec; std::vector<char> h, s, q; };
  auto load = [&](size_t b, uint32_t i, Mate& m) {                  // record + text of read i of batch b
    smr_batch_select(r.gpu, (int)b);
    const size_t len = smr_result_record(r.gpu, i, nullptr, 0);
    m.rec.resize(len);
    if (len) smr_result_record(r.gpu, i, m.rec.data(), len);
    if (feed) {
      size_t tl[3];
      smr_reads_record_text(r.rf[b], i, nullptr, 0, nullptr, 0, nullptr, 0, tl);
      m.h.resize(tl[0] + 1); m.s.resize(tl[1] + 1); m.q.resize(tl[2] + 1);
      smr_reads_record_text(r.rf[b], i, m.h.data(), m.h.size(), m.s.data(), m.s.size(), m.q.data(), m.q.size(), tl);
    }
    if (len) {
      const std::string key = std::to_string(b) + "_" + std::to_string(i);      // KVDB key: <reads file>_<read number>
      put(key.data(), key.size(), m.rec.data(), len);
    }
  };
  Mate m1, m2;
  if (r.paired) {
    const uint32_t np = r.rf.size() == 2 ? smr_reads_count(r.rf[0]) : smr_reads_count(r.rf[0]) / 2;
    for (uint32_t i = 0; i < np; i++) {
      if (r.rf.size() == 2) { load(0, i, m1); load(1, i, m2); } else { load(0, 2 * i, m1); load(0, 2 * i + 1, m2); }
      if (feed && smr_report_add_pair(rep, m1.h.data(), m1.s.data(), is_fastq ? m1.q.data() : nullptr, m1.rec.data(), m1.rec.size(),
                                      m2.h.data(), m2.s.data(), is_fastq ? m2.q.data() : nullptr, m2.rec.data(), m2.rec.size()) != SMR_OK) die(smr_report_last_error(rep));
    }
  } else {
    for (uint32_t i = 0; i < smr_reads_count(r.rf[0]); i++) {
      load(0, i, m1);
      if (feed && smr_report_add(rep, m1.h.data(), m1.s.data(), is_fastq ? m1.q.data() : nullptr, m1.rec.data(), m1.rec.size()) != SMR_OK) die(smr_report_last_error(rep));
    }
  }
  std::vector<uint64_t> cb(2 + n_dbs);
  ctr.assign(2 + n_dbs, 0);
  for (size_t b = 0; b < r.rf.size(); b++) {
    smr_batch_select(r.gpu, (int)b);
    smr_counters(r.gpu, cb.data(), (uint32_t)n_dbs);
    for (size_t k = 0; k < ctr.size(); k++) ctr[k] += cb[k];
  }
  // readstats.store_to_db(kvdb) (processor.cpp:283-284): one more KVDB entry, key = hash of the read files' names
  const char* rfn[2] = {o.reads_paths[0].c_str(), o.reads_paths.size() > 1 ? o.reads_paths[1].c_str() : nullptr};
  char key[32];
  const uint64_t kl = smr_readstats_key(rfn, (uint32_t)o.reads_paths.size(), key, sizeof key);
  std::vector<uint8_t> rs(smr_readstats_record(r.n, r.total_len, r.min_len, r.max_len, ctr[0], ctr[1], ctr.data() + 2, (uint32_t)n_dbs, nullptr, 0));
  smr_readstats_record(r.n, r.total_len, r.min_len, r.max_len, ctr[0], ctr[1], ctr.data() + 2, (uint32_t)n_dbs, rs.data(), rs.size());
  put(key, kl, rs.data(), rs.size());
  fseek(f, 0, SEEK_SET); fwrite(&nrec, 8, 1, f); fclose(f);
  return nrec;
}

// Readstats -> summary.txt
void write_summary(const Run& r, const Options& o, const std::vector<Db>& dbs, const std::vector<uint64_t>& ctr, const uint64_t idc[4], uint64_t total_otu) {
  const std::string sp = o.out_dir + "/summary.txt";
  FILE* f = fopen(sp.c_str(), "w");
  if (!f) die("cannot write " + sp);
  fprintf(f, "Total reads = %llu\nTotal reads passing E-value threshold = %llu\nToo short reads (last part) = %llu\n", (ull)r.n, (ull)ctr[0], (ull)ctr[1]);
  for (size_t k = 0; k < dbs.size(); k++) fprintf(f, "%s\t%llu\n", dbs[k].fasta.c_str(), (ull)ctr[2 + k]);
  if (o.idcov()) fprintf(f, "num_yid_ycov = %llu\nnum_yid_ncov = %llu\nnum_nid_ycov = %llu\nnum_denovo = %llu\nTotal OTUs = %llu\n", (ull)idc[0], (ull)idc[1], (ull)idc[2],
                         (ull)idc[3], (ull)total_otu);
  fclose(f);
}

// aligned.log (Summary::write, summary.cpp:57-100)
void write_log(const Run& r, const Options& o, const std::vector<Db>& dbs, const std::vector<uint64_t>& ctr, const uint64_t idc[4], uint64_t total_otu) {
  const smr_params& base = o.base;
  std::vector<smr_summary_db> sdb(dbs.size());
  for (size_t k = 0; k < dbs.size(); k++) {
    const uint32_t lnwin = dbs[k].info.lnwin;
    sdb[k].ref_file = dbs[k].fasta.c_str();
    sdb[k].skiplengths[0] = lnwin; sdb[k].skiplengths[1] = lnwin / 2; sdb[k].skiplengths[2] = 3;
    sdb[k].lambda = dbs[k].lambda; sdb[k].K = dbs[k].K;
    sdb[k].minimal_score = dbs[k].minimal_score;
    sdb[k].reads_matched = ctr[2 + k];
  }
  const time_t now = time(nullptr);
  const std::string stamp = ctime(&now);
  const char* rfn[2] = {o.reads_paths[0].c_str(), o.reads_paths.size() > 1 ? o.reads_paths[1].c_str() : nullptr};
  smr_summary sm; memset(&sm, 0, sizeof sm);
  sm.cmdline = o.cmdline.c_str(); sm.pid = ""; sm.timestamp = stamp.c_str();
  sm.seed_len = 18; sm.num_seeds = base.num_seeds; sm.edges = base.edges; sm.match = base.match; sm.mismatch = base.mismatch;
  sm.gap_open = base.gap_open; sm.gap_ext = base.gap_ext; sm.score_N = base.score_N; sm.sam_sq = o.ro.sam_sq; sm.threads = 1;
  sm.reads_files = rfn; sm.n_reads_files = (uint32_t)o.reads_paths.size();
  sm.total_reads = r.n; sm.num_aligned = ctr[0]; sm.all_reads_len = r.total_len;
  sm.min_read_len = r.min_len; sm.max_read_len = r.max_len;
  sm.dbs = sdb.data(); sm.n_dbs = (uint32_t)sdb.size();
  sm.is_denovo = o.ro.denovo; sm.total_denovo = idc[3]; sm.is_otu_map = o.ro.otu_map; sm.total_id_cov = idc[0]; sm.total_otu = total_otu;
  if (smr_summary_write((o.out_dir + "/aligned.log").c_str(), &sm) != SMR_OK) die("cannot write aligned.log");
}
}  // namespace

int main(int argc, char** argv) {
  Options o = parse_options(argc, argv);
  check_options(o);
  std::vector<Db>& dbs = o.dbs;
  Run r;
  load_reads(o, r);
  load_indexes(r, o.evalue, dbs);
  upload_reads(o, r);
  size_t n_parts_all = 0;
  for (auto& d : dbs) n_parts_all += d.parts.size();
  // one part in all: it stays resident for the pass and for smr_rows_part / smr_pairwise_part / smr_otu_part
  const bool keep_part = (o.rows_dev() || o.pair_dev() || o.idcov()) && n_parts_all == 1;
  align_parts(r, o, dbs, keep_part);
  uint64_t idc[4] = {0, 0, 0, 0}, total_otu = 0;
  if (o.idcov()) idcov_parts(r, o, dbs, keep_part, idc);
  for (size_t b = 0; b < r.rf.size(); b++) if (smr_batch_select(r.gpu, (int)b) != SMR_OK || smr_results_fetch(r.gpu) != SMR_OK) die(smr_last_error(r.gpu));
  smr_report* rep = o.report() ? open_report(r, o, dbs, &total_otu) : nullptr;
  if (o.split_fx()) fastx_stage(r, o, rep, kSplit, fx_opts(o.ro, r.rf.size() == 2 ? 2 : r.paired ? 1 : 0, true));
  if (o.rows_dev() || o.pair_dev() || o.map_dev()) visit_parts(r, o, dbs, keep_part, rep);
  if (o.dn_dev()) fastx_stage(r, o, rep, kDenovo, fx_opts(o.ro, o.otu_mates_device ? 2 : r.paired ? 1 : 0, false));
  std::vector<uint64_t> ctr;
  const uint64_t nrec = write_records(r, o, dbs.size(), rep, ctr);
  if (rep && smr_report_close(rep) != SMR_OK) die("cannot write the report files");
  write_summary(r, o, dbs, ctr, idc, total_otu);
  write_log(r, o, dbs, ctr, idc, total_otu);
  printf("%llu reads, %llu aligned, %llu records -> %s/records.bin\n", (ull)r.n, (ull)ctr[0], (ull)nrec, o.out_dir.c_str());
  for (auto& d : dbs) for (auto* ix : d.parts) smr_index_free(ix);
  for (auto* rd : r.rf) smr_reads_free(rd);
  smr_destroy(r.gpu);
  return 0;
}
