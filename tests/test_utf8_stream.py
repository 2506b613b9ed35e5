"""kuma_amd/csrc/kmws_utf8_stream.hpp -- the host path's UTF-8 message state
(kmws_decoder_set_utf8_check): the parse-time half (header byte 0 and a frame's
last three bytes -> its view, the stream state advanced) and the delivery-time
half (view + the device's bad bit -> KMWS_UTF8_*) -- checked on the host:
tests/cpp/utf8_stream_check.cpp drives the same inline functions the decoder
calls over every string of length 1-4 over the boundary alphabet of
utf8_rule_check.cpp, cut into 1-4 fragments at every non-decreasing choice of
cut positions (empty fragments included), with and without a PING between any
two, against a sequential decoder restated in the program; then a message
sequence, a dropped generation and a reset.  Host code with its own main, built
once plain and once under ASan + UBSan."""
import os
import subprocess
from math import comb

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "utf8_stream_check.cpp")
# a string of length L is cut into k fragments by k - 1 non-decreasing cuts in [0, L]:
# C(L + k - 1, k - 1) ways; each runs without and with PINGs
EXPECTED_CASES = 2 * sum(24 ** L * sum(comb(L + k - 1, k - 1) for k in range(1, 5)) for L in range(1, 5))


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_utf8_stream_matches_the_restated_decoder(tmp_path, sanitize):
    exe = tmp_path / "utf8_stream_check"
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host",
             "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-Wall", "-Werror",
                           "-Wno-unused-function", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "kuma_amd", "csrc"), SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"OK {EXPECTED_CASES} cases", r.stdout + r.stderr
