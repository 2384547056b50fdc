"""The bodies of test_gpu_rows.py on the emulator (the kernel sources compiled for the host, tests/emu): k_rows_stat, k_rows_size, k_rows_write
and the number formatter without a GPU.  Same bodies, another library behind the binding; device memory lies between guard pages there, so a
store behind the last row's last byte faults at once.  The report side of the feature (smr_report_add_rows) needs no device at all."""
import pytest

from helpers import emu
from test_gpu_rows import COUNTS, WORKLOADS, columns_body, crafted_body, fmt_body, guards_body, report_side_body, workload_body


@pytest.fixture(scope="module", autouse=True)
def emulator():
    with emu.active() as lib:
        yield lib


@pytest.mark.parametrize("fastq", [False, True], ids=["fasta", "fastq"])
@pytest.mark.parametrize("n", COUNTS)
def test_crafted_rows_equal_the_host_writer(n, fastq, tmp_path):
    crafted_body(n, fastq, tmp_path, seed=n)


def test_a_row_longer_than_the_window_next_to_short_rows(tmp_path):
    crafted_body(70, True, tmp_path, seed=5, long_read=True)


def test_blast_columns_in_every_order_and_subset(tmp_path):
    columns_body(tmp_path)


@pytest.mark.parametrize("case", WORKLOADS)
def test_workload_rows_equal_the_host_loop(case, tmp_path):
    workload_body(case, tmp_path)


def test_the_device_formatter_prints_what_printf_prints():
    fmt_body(400)


def test_guards_and_refusals(tmp_path):
    guards_body(tmp_path)


def test_report_add_rows_refusals(tmp_path):
    report_side_body(tmp_path)
