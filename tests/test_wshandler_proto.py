"""tests/cpp/wshandler_proto.cpp: the C++ drop-in's protocol check
(kmws::BasicWSHandler::setProtocolCheck / lastFrameProto,
include/kmws_wshandler.hpp) consumed the way kuma's C++ would: a connection
that is clean up to a CLOSE with a cut reason, one that interleaves a data head,
RSV1 negotiated and not; on the host with unmasked frames, and on the GPU with
masked ones, with and without an RxLoop."""
import os
import subprocess

import pytest

from kuma_amd import build as kb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _build(tmp_path):
    lib = kb.build()
    exe = tmp_path / "wshandler_proto"
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-O2", "-I", INC,
                           os.path.join(ROOT, "tests", "cpp", "wshandler_proto.cpp"),
                           "-L", os.path.dirname(lib), "-lkmws_gpu",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(exe)])
    return exe


def test_wshandler_proto_host(tmp_path):
    """CLIENT mode, unmasked frames: the check runs in the parser, no GPU."""
    r = subprocess.run([str(_build(tmp_path)), "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_wshandler_proto_on_gpu(tmp_path):
    """SERVER mode, masked frames: synchronously and through an RxLoop (async
    and sync), two connections sharing generations; all 0 with the check off."""
    r = subprocess.run([str(_build(tmp_path)), "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
