"""kuma_amd/csrc/kmws_proto_rule.hpp, kmws_proto_stream.hpp and the proto layout
of kmws_workspace.hpp, checked on the host: tests/cpp/proto_rule_check.cpp runs
the very functions the kernels and the decoder call -- proto_compose over all
256^3 triples (associative; identity; constants), every sequence of 1-6 frames
over a 14-frame boundary alphabet from each of the 4 carried states (a scan by
proto_compose + proto_verdict, and the host stream, against a sequential walk
restated in the program), the CLOSE body rule on masked bytes, and the
workspace layout over the sweep of n and n_streams that
tests/golden/make_workspace_sizes.py uses.  Host code with its own main, built
once plain and once under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "proto_rule_check.cpp")
ALPHABET, CARRIES = 14, 4
# triples + (sequences x carried states) + masked CLOSE bodies (3 x 4 keys, and the 125-byte one) + layout points
EXPECTED_CASES = 256 ** 3 + CARRIES * sum(ALPHABET ** n for n in range(1, 7)) + 3 * 4 + 1 + 12 * 4


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_proto_rule_matches_the_restated_walk(tmp_path, sanitize):
    exe = tmp_path / "proto_rule_check"
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
    import proto_util
    f = proto_util.block_frames()
    assert f >= 256 and f % 256 == 0  # whole lanes of a 256-lane block
