"""kmws::tile_of_block (kuma_amd/csrc/kmws_common.hpp), the block -> tile
mapping of the unmask apply grid, checked on the host: tests/cpp/
tile_of_block_check.cpp calls the same inline function the kernel calls, for
every placement kind and nfull in {0, 1, 7, 8, 63, 64, 127, 128, 129, 131,
1000, 4099, 32768 + 7}, and requires a permutation of [0, nfull) equal to the
division formulas the function replaced (restated in the program).  Host code
with its own main, built once plain and once under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tile_of_block_check.cpp")
EXPECTED_BLOCKS = 6 * sum([0, 1, 7, 8, 63, 64, 127, 128, 129, 131, 1000, 4099, 32768 + 7])


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_tile_of_block_is_the_parent_permutation(tmp_path, sanitize):
    exe = tmp_path / "tile_of_block_check"
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host",
             "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    # the header is HIP source (hip_runtime.h, __host__ __device__): hipcc, host side only
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-Wall", "-Werror",
                           "-Wno-unused-function", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "kuma_amd", "csrc"), SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"OK {EXPECTED_BLOCKS} blocks", r.stdout + r.stderr
