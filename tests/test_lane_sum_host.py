"""Builds and runs tests/cpp/test_lane_sum.cpp: the header that decides how many terms a lane of a big round adds into its running sums
(sumcheck_amd/csrc/lane_sum.hpp) compiled for the HOST under AddressSanitizer and UndefinedBehaviorSanitizer, against the kernel's loops
restated lane by lane -- a stand-alone program.  lane_table() is its enumeration of every big round the library admits, for the exact model
of the accumulator (tests/test_fe_model_host.py)."""
import functools
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_lane_sum.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "test_lane_sum.bin")


def build_lane_sum():
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "sumcheck_amd", "csrc"), SRC, "-o", BIN]
    subprocess.check_call(cmd)
    return BIN


@functools.lru_cache(maxsize=None)
def lane_table():
    """-> rows (nv, round, rows, M, grid, terms, two_pairs): rows = 0 one launch per product, else the merged launch of that many products;
    terms: what the busiest lane adds into one running sum, two_pairs: whether a term holds two pairs' products -- by the library's own rules"""
    out = subprocess.run([build_lane_sum(), "--table"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]


def test_lane_sum_header_on_the_host_under_sanitizers():
    out = subprocess.run([build_lane_sum()], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL TESTS PASSED" in out.stdout


def test_the_enumeration_covers_every_big_round():
    rows = lane_table()
    assert len(rows) == sum(nv - 15 for nv in range(15, 41)) * 6 * 4
    assert {r[0] for r in rows} == set(range(16, 41)) and max(r[1] for r in rows) == 25
    assert all(1 <= r[4] <= 1024 and r[5] >= 1 for r in rows)
