"""kuma_amd/csrc/kmws_workspace.hpp -- where everything lies in a caller
workspace -- checked on the host.

tests/cpp/workspace_layout_check.cpp calls the layout functions over a sweep
and checks alignment, bounds, overlap, capacity for the launchers' counts,
64-bit wrap and the composition of the layouts.  Host code with its own main,
built once plain and once under ASan + UBSan, run as a child process.

tests/golden/workspace_sizes.json pins every kmws_*_workspace_size over the
same sweep to the values of the library before the layouts had one home
(tests/golden/make_workspace_sizes.py wrote it from that library)."""
import ctypes
import importlib.util
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "workspace_layout_check.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")

_spec = importlib.util.spec_from_file_location(
    "make_workspace_sizes", os.path.join(ROOT, "tests", "golden", "make_workspace_sizes.py"))
sweep = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(sweep)

N, MEANS, SPANS, STREAMS = len(sweep.NS), len(sweep.MEANS), len(sweep.SPANS), 4
EXPECTED_CASES = (
    SPANS                          # the unmask plan
    + SPANS * N * STREAMS * 2      # UTF-8 validate, fused unmask + UTF-8
    + N * MEANS * 2                # copy, reframe
    + N * MEANS * STREAMS * 2      # validating gather, validating reframe
    + N                            # pack-headers
)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_workspace_layouts_hold_over_the_sweep(tmp_path, sanitize):
    exe = tmp_path / "workspace_layout_check"
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host",
             "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-Wall", "-Werror",
                           "-Wno-unused-function", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "kuma_amd", "csrc"), SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"OK {EXPECTED_CASES} cases", r.stdout + r.stderr


def test_workspace_sizes_match_the_pinned_rows():
    from kuma_amd import build as kb
    with open(GOLDEN) as f:
        want = json.load(f)
    assert set(want) == set(sweep.SWEEPS)
    got = sweep.rows(ctypes.CDLL(kb.build()))
    for name, rows in want.items():
        assert len(rows) == len(sweep.SWEEPS[name][1]), name
        bad = [(w, g) for w, g in zip(rows, got[name]) if w != g]
        assert not bad, f"{name}: {len(bad)} rows differ, first (pinned, now): {bad[0]}"
