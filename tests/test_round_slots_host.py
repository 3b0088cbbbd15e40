"""The slot rule of the big rounds without a GPU.  tests/cpp/test_round_slots.cpp: the header every launch plan of protocol.hip builds its
kernel slots by (sumcheck_amd/csrc/round_slots.hpp), compiled for the HOST under AddressSanitizer and UndefinedBehaviorSanitizer -- a
stand-alone program that enumerates every list of one to three products over three tables, every prior table state, bind on and off, one
launch for the round and one launch per product, and checks what a round must keep: which buffer every slot reads and stores, in which
format, and where the tables stand afterwards."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_round_slots.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "test_round_slots.bin")


def build_round_slots():
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "sumcheck_amd", "csrc"), SRC, "-o", BIN]
    subprocess.check_call(cmd)
    return BIN


def test_round_slots_header_on_the_host_under_sanitizers():
    out = subprocess.run([build_round_slots()], capture_output=True, text=True, timeout=120)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL TESTS PASSED" in out.stdout


def test_the_build_knows_the_header():
    from sumcheck_amd import build
    assert "round_slots.hpp" in build.HEADERS
