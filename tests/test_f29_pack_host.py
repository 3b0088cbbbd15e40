"""Builds and runs tests/cpp/test_f29_pack.cpp: the packed table format's header (sumcheck_amd/csrc/f29_pack.hpp) compiled for the HOST
under AddressSanitizer and UndefinedBehaviorSanitizer, against a big-integer restatement.  A stand-alone program; no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_f29_pack.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "test_f29_pack.bin")


def build_f29_pack():
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "sumcheck_amd", "csrc"), SRC, "-o", BIN]
    subprocess.check_call(cmd)
    return BIN


def test_f29_pack_header_on_the_host_under_sanitizers():
    out = subprocess.run([build_f29_pack()], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL TESTS PASSED" in out.stdout
