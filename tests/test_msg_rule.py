"""kuma_amd/csrc/kmws_msg_rule.hpp and the msg layout of kmws_workspace.hpp,
checked on the host: tests/cpp/msg_rule_check.cpp runs the very functions the
kernels of kmws_msg_index call -- msg_compose over all triples of an 18-value
domain (associative; identity; constants; applies like its parts),
msg_sum_compose over 200,000 random triples with byte totals past 2^32, every
sequence of 1-6 frames over a 9-frame boundary alphabet from each of 3 kinds of
carry (both scans and the records taken at the reset points, against a
sequential walk restated in the program), and the workspace layout over the
sweep of n and n_streams.  Host code with its own main, built once plain and
once under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "msg_rule_check.cpp")
DOMAIN, TRIPLES, ALPHABET, CARRIES = 18, 200000, 9, 3
EXPECTED_CASES = DOMAIN ** 3 + TRIPLES + CARRIES * sum(ALPHABET ** n for n in range(1, 7)) + 12 * 4


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_msg_rule_matches_the_restated_walk(tmp_path, sanitize):
    exe = tmp_path / "msg_rule_check"
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host",
             "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-Wall", "-Werror",
                           "-Wno-unused-function", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "kuma_amd", "csrc"), SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"OK {EXPECTED_CASES} cases", r.stdout + r.stderr


def test_block_frames_constant_is_exported():
    """The tests size their scan shapes from it."""
    import msg_util
    f = msg_util.block_frames()
    assert f >= 256 and f % 256 == 0  # whole lanes of a 256-lane block
