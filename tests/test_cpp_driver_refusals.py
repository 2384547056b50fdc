"""The C++ host driver (examples/smr_align.cpp): every refusal it raises before it loads anything -- while it reads the command line, and in the
checks between the command line and the first file.  Each row is a command line and the message that must end it: a non-zero exit, that
message on stderr, and nothing written to --out.  Where two refusals hold for one command line, a row pins which of them is reported: the
checks run in a fixed order."""
import os
import subprocess

import pytest

from test_cpp_driver import _emu_driver
from test_cpp_split_device import _paired_args

SWITCHES = ["pack", "split", "rows", "pairwise", "unzip", "zip", "ziprows", "mates", "otu-mates", "otu"]
TWO = _paired_args()                     # --ref DB --gumbel LAMBDA K --reads MATES_1 --reads MATES_2
ONE = TWO[:-2]
REF, READS = TWO[:5], TWO[5:7]
PACK = ["--pack", "device"]

MATES_TWO_FILES = "--mates device interleaves the rows of mates in two reads files on the device: it needs two --reads files"
MATES_ROWS = "--mates device interleaves what --rows device and --pairwise device write for two reads files: it needs one of the two"
SPLIT_PACK = "--split device writes aligned.* / other.* from the text the device parsed: it needs --pack device"
UNZIP_PACK = "--unzip device inflates a gzip reads file into the text buffer the device parses: it needs --pack device"
ROWS_PACK = "--rows device writes the SAM / BLAST rows from the text the device parsed: it needs --pack device"
PAIR_PACK = "--pairwise device writes the BLAST pairwise text from the text the device parsed: it needs --pack device"
PAIR_BLAST0 = "--pairwise device writes the pairwise text of --blast 0: without --blast 0 there is none"
PAIR_ONE_FILE = ("--pairwise device takes one reads file (single reads or interleaved mates): the blocks of mates in two files alternate between "
                 "the batches and stay with --pairwise host")
ROWS_BLAST0 = "--rows device writes BLAST tabular rows only: --blast 0 (pairwise) stays with --rows host"
ROWS_ONE_FILE = ("--rows device takes one reads file (single reads or interleaved mates): the rows of mates in two files alternate between the "
                 "batches and stay with --rows host")
ID_COV_ALONE = "options '-id' and '-coverage' can only be used together with '-otu_map': they are the thresholds of the OTU map"
OTU_NO_BEST = "option '-otu_map' cannot be used with '-no-best': the OTU map is built from the best alignments"
ID_COV_RANGE = "-id and -coverage take a value within [0, 1]"
OTU_PACK = "--otu device writes the OTU map and aligned_denovo.* from the text the device parsed: it needs --pack device"
OTU_ONE_FILE = ("--otu device takes one reads file (single reads or interleaved mates): the members of a group of mates in two files alternate "
                "between the batches and stay with --otu host")
OTU_MATES_TWO_FILES = "--otu-mates device writes the OTU map and aligned_denovo.* of mates in two reads files on the device: it needs two --reads files"
OTU_MATES_PACK = "--otu-mates device writes the OTU map and aligned_denovo.* from the text the device parsed: it needs --pack device"
REQUIRED = "--ref and --reads are required (see --help)"
PARAMS = ("these options are outside what libsmr_hip aligns (the reference accepts them): edges must be 1..10 (nucleotides or percent), like the "
          "reference's --edges")
GUMBEL = "--gumbel LAMBDA K is required after every --ref (see --help): the values of the reference's log for this DB and scoring scheme"
ZIP_SPLIT = "--zip device compresses the aligned.* / other.* streams where --split device leaves them: it needs --split device"
ZIP_PLAIN = "--zip device writes gzip members: the reports of this run are not gzipped (a plain reads file without -zip-out 1, or -zip-out 0)"
ZIPROWS_ROWS = ("--ziprows device compresses the SAM / BLAST rows and the pairwise text where --rows device and --pairwise device leave them: it "
                "needs one of the two")
ZIPROWS_PLAIN = "--ziprows device writes gzip members: the reports of this run are not gzipped (a plain reads file without -zip-out 1, or -zip-out 0)"
BLAST_VALUE = "-blast: '0' (pairwise) or '1 [cigar] [qcov] [qstrand]' (tabular)"

CASES = [
    # ---- while the command line is read
    ("missing_value_last", ONE + ["--reads"], "missing value after --reads"),
    ("missing_value_switch", ONE + ["--pack"], "missing value after --pack"),
    ("missing_value_second_of_gumbel", ["--ref", "db.fa", "--gumbel", "0.6"], "missing value after --gumbel"),
    ("unknown_option", ONE + ["--frobnicate"], "unknown option --frobnicate"),
    ("unknown_option_wins_over_later_ones", ["--frobnicate", "--split", "sometimes"], "unknown option --frobnicate"),
    ("idx_before_ref", ["--idx", "prefix"], "--idx before --ref"),
    ("gumbel_before_ref", ["--gumbel", "0.6", "0.33"], "--gumbel before --ref"),
    ("third_reads", TWO + ["--reads", "third.fq"], "at most two --reads files (mates)"),
    ("third_reads_before_its_value", TWO + ["--reads"], "at most two --reads files (mates)"),
    ("blast_value", ONE + ["--blast", "2"], BLAST_VALUE),
    ("blast_empty", ONE + ["-blast", ""], BLAST_VALUE),
    ("blast_columns", ONE + ["--blast", "1 " + "cigar " * 13], "-blast: too many columns"),
    ("first_bad_option_wins", ["--idx", "prefix", "--frobnicate"], "--idx before --ref"),
] + [
    ("%s_%s_value" % ("two_dashes" if dashes == "--" else "one_dash", name), ONE + [dashes + name, "sometimes"], "--%s: host or device" % name)
    for name in SWITCHES for dashes in ("-", "--")
] + [
    # ---- between the command line and the first file, in the order of the checks
    ("mates_one_file", ONE + PACK + ["--rows", "device", "--mates", "device", "--sam"], MATES_TWO_FILES),
    ("mates_one_file_wins_over_no_rows", ONE + PACK + ["--mates", "device", "--sam"], MATES_TWO_FILES),
    ("mates_without_rows_or_pairwise", TWO + PACK + ["--mates", "device", "--sam"], MATES_ROWS),
    ("mates_without_rows_wins_over_split_without_pack", TWO + ["--mates", "device", "--split", "device"], MATES_ROWS),
    ("split_without_pack", ONE + ["--split", "device"], SPLIT_PACK),
    ("split_pack_host", ONE + ["--split", "device", "--pack", "host"], SPLIT_PACK),
    ("split_wins_over_unzip_rows_pairwise", ONE + ["--pairwise", "device", "--rows", "device", "--unzip", "device", "--split", "device"], SPLIT_PACK),
    ("split_wins_over_missing_inputs", ["--split", "device"], SPLIT_PACK),
    ("unzip_without_pack", ONE + ["--unzip", "device"], UNZIP_PACK),
    ("unzip_wins_over_rows", ONE + ["--rows", "device", "--unzip", "device"], UNZIP_PACK),
    ("rows_without_pack", ONE + ["--rows", "device", "--sam"], ROWS_PACK),
    ("rows_wins_over_pairwise", ONE + ["--pairwise", "device", "--rows", "device", "--blast", "0"], ROWS_PACK),
    ("rows_without_pack_wins_over_two_files", TWO + ["--rows", "device", "--sam"], ROWS_PACK),
    ("pairwise_without_pack", ONE + ["--pairwise", "device", "--blast", "0"], PAIR_PACK),
    ("pairwise_without_pack_wins_over_no_blast0", ONE + ["--pairwise", "device"], PAIR_PACK),
    ("pairwise_without_blast0", ONE + PACK + ["--pairwise", "device"], PAIR_BLAST0),
    ("pairwise_with_tabular_only", ONE + PACK + ["--pairwise", "device", "--blast", "1"], PAIR_BLAST0),
    ("pairwise_without_blast0_wins_over_two_files", TWO + PACK + ["--pairwise", "device"], PAIR_BLAST0),
    ("pairwise_two_files", TWO + PACK + ["--pairwise", "device", "--blast", "0"], PAIR_ONE_FILE),
    ("pairwise_two_files_mates_host", TWO + PACK + ["--pairwise", "device", "--blast", "0", "--mates", "host"], PAIR_ONE_FILE),
    ("pairwise_two_files_wins_over_rows_two_files", TWO + PACK + ["--rows", "device", "--pairwise", "device", "--blast", "0", "--sam"], PAIR_ONE_FILE),
    ("rows_blast0", ONE + PACK + ["--rows", "device", "--blast", "0"], ROWS_BLAST0),
    ("rows_blast0_wins_over_two_files", TWO + PACK + ["--rows", "device", "--blast", "0"], ROWS_BLAST0),
    ("rows_two_files", TWO + PACK + ["--rows", "device", "--sam"], ROWS_ONE_FILE),
    ("rows_two_files_mates_host", TWO + PACK + ["--rows", "device", "--sam", "--mates", "host"], ROWS_ONE_FILE),
    ("rows_two_files_wins_over_id_alone", TWO + PACK + ["--rows", "device", "--sam", "-id", "0.9"], ROWS_ONE_FILE),
    ("id_without_otu_map", ONE + ["-id", "0.9"], ID_COV_ALONE),
    ("coverage_without_otu_map", ONE + ["--coverage", "0.9"], ID_COV_ALONE),
    ("id_alone_wins_over_its_range", ONE + ["-id", "1.5"], ID_COV_ALONE),
    ("otu_map_no_best", ONE + ["-otu_map", "-no-best"], OTU_NO_BEST),
    ("otu_map_no_best_wins_over_range", ONE + ["-otu_map", "-no-best", "-id", "1.5"], OTU_NO_BEST),
    ("id_range", ONE + ["-otu_map", "-id", "1.5"], ID_COV_RANGE),
    ("coverage_range", ONE + ["-otu_map", "-coverage", "-0.1"], ID_COV_RANGE),
    ("id_not_a_number", ONE + ["-otu_map", "-id", "nan"], ID_COV_RANGE),
    ("range_wins_over_otu_without_pack", ONE + ["-otu_map", "-id", "1.5", "--otu", "device"], ID_COV_RANGE),
    ("otu_without_pack", ONE + ["-otu_map", "--otu", "device"], OTU_PACK),
    ("otu_without_pack_wins_over_two_files", TWO + ["-otu_map", "--otu", "device"], OTU_PACK),
    ("otu_two_files", TWO + PACK + ["-otu_map", "--otu", "device"], OTU_ONE_FILE),
    ("otu_two_files_after_the_mates_checks", TWO + PACK + ["--rows", "device", "--mates", "device", "--sam", "-otu_map", "--otu", "device"], OTU_ONE_FILE),
    ("otu_two_files_wins_over_otu_mates_without_pack", TWO + PACK + ["-otu_map", "--otu", "device", "--otu-mates", "device"], OTU_ONE_FILE),
    ("otu_mates_one_file", ONE + PACK + ["-otu_map", "--otu-mates", "device"], OTU_MATES_TWO_FILES),
    ("otu_mates_one_file_wins_over_pack", ONE + ["-otu_map", "--otu-mates", "device"], OTU_MATES_TWO_FILES),
    ("otu_mates_without_pack", TWO + ["-otu_map", "--otu-mates", "device"], OTU_MATES_PACK),
    ("otu_mates_without_pack_wins_over_edges", TWO + ["--otu-mates", "device", "-edges", "0"], OTU_MATES_PACK),
    ("nothing_given", [], REQUIRED),
    ("no_reads", REF, REQUIRED),
    ("no_ref", READS, REQUIRED),
    ("required_wins_over_edges", READS + ["-edges", "0"], REQUIRED),
    ("required_wins_over_gumbel", ["--ref", "db.fa"], REQUIRED),
    ("edges_below", ONE + ["-edges", "0"], PARAMS),
    ("edges_above", ONE + ["--edges", "11"], PARAMS),
    ("edges_wins_over_gumbel", ["--ref", "db.fa"] + READS + ["-edges", "0"], PARAMS),
    ("no_gumbel", ["--ref", "db.fa"] + READS, GUMBEL),
    ("no_gumbel_after_the_second_ref", ONE + ["--ref", "db2.fa"], GUMBEL),
    ("no_gumbel_wins_over_zip", ["--ref", "db.fa"] + READS + PACK + ["--zip", "device"], GUMBEL),
    # ---- after the first reads file's first two bytes have said whether the reports are gzipped
    ("zip_without_split", ONE + PACK + ["--zip", "device", "-zip-out", "1"], ZIP_SPLIT),
    ("zip_without_split_wins_over_plain_reports", ONE + PACK + ["--zip", "device"], ZIP_SPLIT),
    ("zip_without_split_wins_over_ziprows", ONE + PACK + ["--zip", "device", "--ziprows", "device"], ZIP_SPLIT),
    ("zip_plain_reads_file", ONE + PACK + ["--split", "device", "--zip", "device", "--fastx"], ZIP_PLAIN),
    ("zip_with_zip_out_0", ONE + PACK + ["--split", "device", "--zip", "device", "--fastx", "-zip-out", "0"], ZIP_PLAIN),
    ("zip_plain_wins_over_ziprows", ONE + PACK + ["--split", "device", "--zip", "device", "--ziprows", "device"], ZIP_PLAIN),
    ("ziprows_without_rows_or_pairwise", ONE + PACK + ["--ziprows", "device", "-zip-out", "1"], ZIPROWS_ROWS),
    ("ziprows_without_rows_wins_over_plain_reports", ONE + PACK + ["--ziprows", "device"], ZIPROWS_ROWS),
    ("ziprows_plain_reads_file", ONE + PACK + ["--rows", "device", "--sam", "--ziprows", "device"], ZIPROWS_PLAIN),
    ("ziprows_pairwise_with_zip_out_0", ONE + PACK + ["--pairwise", "device", "--blast", "0", "--ziprows", "device", "--zip-out", "no"], ZIPROWS_PLAIN),
]


@pytest.fixture(scope="module")
def exe():
    return _emu_driver()


def test_every_row_has_its_own_name():
    names = [c[0] for c in CASES]
    assert len(set(names)) == len(names)


@pytest.mark.parametrize("args,message", [pytest.param(a, m, id=n) for n, a, m in CASES])
def test_refused_before_anything_is_loaded_or_written(exe, args, message, tmp_path):
    out = tmp_path / "out"
    os.makedirs(out)
    p = subprocess.run([exe, "--out", str(out)] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode != 0
    assert p.stderr.decode() == "ERROR: %s\n" % message
    assert p.stdout == b""
    assert not os.listdir(str(out))
