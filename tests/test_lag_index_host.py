"""The lagging single-table products without a GPU.  tests/cpp/test_lag_index.cpp: the index header (sumcheck_amd/csrc/lag_index.hpp)
compiled for the HOST under AddressSanitizer and UndefinedBehaviorSanitizer, against brute force -- a stand-alone program.  And the
identity the whole scheme rests on, in Python integers: the class table, bound round by round, gives every round the same sum of even and
sum of odd entries as the table itself, and the table bound with all missed challenges at once is the table the rounds would have left."""
import os
import random
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_lag_index.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "test_lag_index.bin")
P = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001


def build_lag_index():
    cmd = ["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", os.path.join(ROOT, "sumcheck_amd", "csrc"), SRC, "-o", BIN]
    subprocess.check_call(cmd)
    return BIN


def test_lag_index_header_on_the_host_under_sanitizers():
    out = subprocess.run([build_lag_index()], capture_output=True, text=True, timeout=600)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL TESTS PASSED" in out.stdout


def bind(tab, r):
    return [(tab[2 * i] + r * (tab[2 * i + 1] - tab[2 * i])) % P for i in range(len(tab) // 2)]


def test_class_table_gives_the_rounds_sums_and_the_catch_up_gives_the_table():
    nv = 8
    rng = random.Random(0x1A6)
    table = [rng.randrange(P) for _ in range(1 << nv)]
    rs = [rng.randrange(P) for _ in range(nv)]
    for j in (3, 4, 5, 6):  # catch-up before round j: rounds 2 .. j - 1 see the class table only
        m = j - 1
        classes = [sum(table[c::1 << m]) % P for c in range(1 << m)]
        full, cls = table, classes
        assert (sum(full[0::2]) % P, sum(full[1::2]) % P) == (sum(cls[0::2]) % P, sum(cls[1::2]) % P)  # round 1
        for rnd in range(2, j):
            full, cls = bind(full, rs[rnd - 2]), bind(cls, rs[rnd - 2])
            assert len(cls) >= 2
            assert (sum(full[0::2]) % P, sum(full[1::2]) % P) == (sum(cls[0::2]) % P, sum(cls[1::2]) % P), (j, rnd)
        deep = table  # k_fix_deep: every missed challenge and round j's own, in order
        for r in rs[:j - 1]:
            deep = bind(deep, r)
        assert deep == bind(full, rs[j - 2])
