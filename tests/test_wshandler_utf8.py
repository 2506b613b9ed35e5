"""tests/cpp/wshandler_utf8.cpp: the C++ drop-in's UTF-8 check
(kmws::BasicWSHandler::setUtf8Check / lastFrameUtf8, include/kmws_wshandler.hpp)
consumed the way kuma's C++ would: one text message BAD, one OK, a code point
straddling fragments, with and without an RxLoop."""
import os
import subprocess

import pytest

from kuma_amd import build as kb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def _build(tmp_path):
    lib = kb.build()
    exe = tmp_path / "wshandler_utf8"
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Wextra", "-Werror", "-O2", "-I", INC,
                           os.path.join(ROOT, "tests", "cpp", "wshandler_utf8.cpp"),
                           "-L", os.path.dirname(lib), "-lkmws_gpu",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", str(exe)])
    return exe


def test_wshandler_utf8_host(tmp_path):
    """Empty frames of a CLIENT-mode handler need no GPU: OK / 0 with the check
    on, 0 with it off."""
    r = subprocess.run([str(_build(tmp_path)), "host"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_wshandler_utf8_on_gpu(tmp_path):
    """SERVER-mode masked text: BAD / AFTER_BAD / OK / 0 per frame inside the
    frame callback, synchronously and through an RxLoop (async and sync), and
    all 0 with the check off."""
    r = subprocess.run([str(_build(tmp_path)), "gpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout + r.stderr
