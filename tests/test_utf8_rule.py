"""kuma_amd/csrc/kmws_utf8_rule.hpp -- the byte rule, the scan operator, the
frame element / view and the carry that the kmws_utf8_validate kernels call --
checked on the host: tests/cpp/utf8_rule_check.cpp drives the same inline
functions over every string of length 1-4 over the boundary alphabet {00, 7F,
80, 8F, 90, 9F, A0, BF, C0, C1, C2, DF, E0, E1, EC, ED, EE, EF, F0, F1, F3, F4,
F5, FF}, under every split into fragments and every cut into two batches joined
by the carry, against a decoder restated in the program; checks the 16-byte
word form of the rule (four bytes per operation, what the payload pass runs on
words inside a frame) against the byte rule on six million random and
near-well-formed windows; and checks the operator's associativity on random
triples.  Host code with its own main, built
once plain and once under ASan + UBSan."""
import os
import subprocess
from math import comb

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "utf8_rule_check.cpp")
# a string of length L splits into f frames in C(L-1, f-1) ways, each run with f + 1 cuts
EXPECTED_CASES = sum(24 ** L * sum(comb(L - 1, f - 1) * (f + 1) for f in range(1, L + 1)) for L in range(1, 5))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_utf8_rule_matches_the_restated_decoder(tmp_path, sanitize):
    exe = tmp_path / "utf8_rule_check"
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host",
             "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-Wall", "-Werror",
                           "-Wno-unused-function", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "kuma_amd", "csrc"), SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"OK {EXPECTED_CASES} cases", r.stdout + r.stderr
