"""Writes tests/golden/workspace_sizes.json: every kmws_*_workspace_size of one
library over the sweep of tests/cpp/workspace_layout_check.cpp, as compact rows
[arguments..., bytes].  The committed file was generated from the library of
the commit before kmws_workspace.hpp, so tests/test_workspace_layout.py pins
the layouts to it byte for byte.  The size functions need no device.

    python tests/golden/make_workspace_sizes.py path/to/libkmws_gpu.so [out.json]
"""
import ctypes
import json
import os
import sys

NS = [0, 1, 2, 255, 256, 257, 2047, 2048, 2049, 65536, 2 ** 20 + 1, 2 ** 31 - 1]
MEANS = [0, 1, 300, 4104, 16383, 16384, 65550]  # dst_cap = n * mean: both sides of the copy-form switch
SPANS = [0, 1, 16383, 16384, 16385, 2 ** 31, 2 ** 32 + 16400, 2 ** 40]


def streams(n):
    return [0, 1, 2, n + 1]


u32, u64 = ctypes.c_uint32, ctypes.c_uint64
# name -> (argument types, argument tuples)
SWEEPS = {
    "kmws_unmask_workspace_size": ((u64,), [(s,) for s in SPANS]),
    "kmws_utf8_workspace_size": ((u64, u32, u32), [(s, n, k) for s in SPANS for n in NS for k in streams(n)]),
    "kmws_unmask_utf8_workspace_size": ((u64, u32, u32), [(s, n, k) for s in SPANS for n in NS for k in streams(n)]),
    "kmws_copy_workspace_size": ((u32, u64), [(n, n * m) for n in NS for m in MEANS]),
    "kmws_reframe_workspace_size": ((u32, u64), [(n, n * m) for n in NS for m in MEANS]),
    "kmws_gather_utf8_workspace_size": ((u32, u64, u32),
                                        [(n, n * m, k) for n in NS for m in MEANS for k in streams(n)]),
    "kmws_reframe_utf8_workspace_size": ((u32, u64, u32),
                                         [(n, n * m, k) for n in NS for m in MEANS for k in streams(n)]),
    "kmws_pack_headers_workspace_size": ((u32,), [(n,) for n in NS]),
    "kmws_unpack_workspace_size": ((), [()]),
}


def rows(lib):
    out = {}
    for name, (argtypes, points) in SWEEPS.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = list(argtypes), ctypes.c_size_t
        out[name] = [[*p, fn(*p)] for p in points]
    return out


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    dst = sys.argv[2] if len(sys.argv) > 2 else os.path.join(here, "workspace_sizes.json")
    with open(dst, "w") as f:
        json.dump(rows(ctypes.CDLL(sys.argv[1])), f, separators=(",", ":"))
        f.write("\n")
