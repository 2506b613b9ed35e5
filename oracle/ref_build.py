"""TEST INFRASTRUCTURE ONLY -- builds the reference's own WSHandler.cpp.

Where the reference checkout is present, `build()` compiles its unmodified
src/ws/WSHandler.cpp together with oracle/ref_wrap.cpp (our extern "C" wrapper
with the oracle's ABI under a ref_ prefix) into

    oracle/_ref/libkmws_ref_O3.so   -O3, the reference's cmake Release flag
    oracle/_ref/libkmws_ref_O0.so   -O0

Two optimisation levels because the 127-class length read of decodeFrame is
undefined behaviour (`data[pos] << 56` on an int): what the compiled code does
with it at both levels is part of what the tests pin.

What the build needs beyond the checkout:
  * oracle/ref_shim/: stand-ins, written from scratch, for the three headers of
    the empty libkev submodule and for http/HttpParserImpl.h;
  * oracle/_ref/include/kmbuffer.h: a copy of the reference's kmbuffer.h with
    the one token changed that keeps the shipped header from compiling (SURVEY
    8 a-15), written here exactly as tests/test_kuma_types.py writes its copy.

Include order: shim, oracle/_ref/include, then the reference's include, src,
src/ws.  oracle/_ref/ is ignored by git: nothing compiled from the reference
is committed.  Where the checkout is absent, `build()` does nothing and leaves
oracle/_ref/ as it is (libraries built elsewhere travel with the tree).
"""
from __future__ import annotations

import os
import subprocess
from typing import Dict, Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("KMWS_REFERENCE_DIR", "/root/reference")
OUT_DIR = os.path.join(_HERE, "_ref")
SHIM_DIR = os.path.join(_HERE, "ref_shim")
WRAP = os.path.join(_HERE, "ref_wrap.cpp")
OPTS = ("O3", "O0")


def lib_path(opt: str, out_dir: Optional[str] = None) -> str:
    assert opt in OPTS, opt
    return os.path.join(out_dir or OUT_DIR, f"libkmws_ref_{opt}.so")


def reference_source(reference: Optional[str] = None) -> str:
    return os.path.join(reference or REFERENCE, "src", "ws", "WSHandler.cpp")


def _patched_kmbuffer(reference: str, inc_dir: str) -> None:
    src = open(os.path.join(reference, "include", "kmbuffer.h")).read()
    bad = "auto* createSharedData("
    assert src.count(bad) == 1, "the known kmbuffer.h defect moved; re-check SURVEY 8 a-15"
    os.makedirs(inc_dir, exist_ok=True)
    with open(os.path.join(inc_dir, "kmbuffer.h"), "w") as f:
        f.write(src.replace(bad, "_SharedBase* createSharedData("))


def build(reference: Optional[str] = None, out_dir: Optional[str] = None) -> Dict[str, str]:
    """Build both libraries; {} (and nothing touched) where the reference is absent."""
    reference = reference or REFERENCE
    out_dir = out_dir or OUT_DIR
    src = reference_source(reference)
    if not os.path.exists(src):
        return {}
    inc_dir = os.path.join(out_dir, "include")
    _patched_kmbuffer(reference, inc_dir)
    includes = [SHIM_DIR, inc_dir, os.path.join(reference, "include"),
                os.path.join(reference, "src"), os.path.join(reference, "src", "ws")]
    built = {}
    for opt in OPTS:
        out = lib_path(opt, out_dir)
        cmd = ["g++", "-std=c++14", f"-{opt}", "-fPIC", "-shared", "-w"]
        for inc in includes:
            cmd += ["-I", inc]
        cmd += [src, WRAP, "-o", out + ".tmp"]
        subprocess.check_call(cmd)
        os.replace(out + ".tmp", out)
        built[opt] = out
    return built


if __name__ == "__main__":
    print(build())
