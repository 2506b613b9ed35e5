"""kuma_amd/csrc/kmws_resident_proto.hpp -- the resident worker's mailbox
format: the job word and its accessors, job_done's half-range rule, the
descriptor and verdict tags, hull_words, the split of a job over its parts and
the host's edge-word pick -- checked on the host: tests/cpp/resident_proto_check.cpp
drives the same inline functions the kernel and ResidentWorker::post call, at
the wrap-arounds no GPU test reaches in its lifetime (40-bit job numbers, 16-
and 11-bit tags) and against brute-force walks of every hull word.  Host code
with its own main, built once plain and once under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "resident_proto_check.cpp")
JOBS, COUNTS, PARTS = 6, 4, 4
EXPECTED_CASES = (
    JOBS * COUNTS * PARTS * 2 ** 5          # pack -> accessors, every combination of the five flags
    + JOBS * COUNTS * PARTS * 4 * 3         # cancel / claimed / quit set and cleared on each write-through x check word
    + 4 * 5                                 # job_done: four job numbers, three done words at or past, two before
    + 9 * 2 * 3 + 9 * 2                     # tags: nine job numbers; descriptors (2 addresses x 3 lengths), verdict words
    + 16 * 50                               # hull_words: address mod 16 x length
    + 5 * 4096 + 1                          # the part split of every total
    + 3 + 1 + 300 + 1                       # edge pick: sixteen-frame reads, one 64 KiB payload, random jobs, explicit
)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_resident_proto_matches_its_restatement(tmp_path, sanitize):
    exe = tmp_path / "resident_proto_check"
    flags = ["-O1", "-g", "-Xarch_host", "-fsanitize=undefined,address", "-Xarch_host",
             "-fno-sanitize-recover=undefined"] if sanitize else ["-O2"]
    subprocess.check_call(["hipcc", "-x", "hip", "--offload-host-only", "-std=c++17", "-Wall", "-Werror",
                           "-Wno-unused-function", *flags, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "kuma_amd", "csrc"), SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=0"})
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"OK {EXPECTED_CASES} cases", r.stdout + r.stderr
