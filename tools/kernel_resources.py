"""Registers, LDS and scratch of every kernel of a source tree, one line per
kernel symbol, from hipcc's -Rpass-analysis=kernel-resource-usage (device code
only, no GPU needed).  Two trees side by side show whether a change touched the
code of kernels it did not mean to:

    python tools/kernel_resources.py                       # this tree
    python tools/kernel_resources.py --root /path/to/other/checkout
"""
import argparse
import glob
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds"))


def resources(src, root, arch):
    cmd = ["hipcc", "-x", "hip", f"--offload-arch={arch}", "--cuda-device-only", "-O3", "-std=c++17",
           "-Rpass-analysis=kernel-resource-usage", "-Wno-unused-function", "-I", os.path.join(root, "include"),
           "-I", os.path.dirname(src), "-c", src, "-o", os.devnull]
    err = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--arch", default="gfx950")
    a = ap.parse_args()
    srcs = sorted(glob.glob(os.path.join(a.root, "kuma_amd", "csrc", "*.hip")))
    with ThreadPoolExecutor(max_workers=4) as ex:
        per = list(ex.map(lambda s: resources(s, a.root, a.arch), srcs))
    for src, res in zip(srcs, per):
        for name in sorted(res):
            sym = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
            r = res[name]
            print(f"{os.path.basename(src)}  {sym}  " + "  ".join(f"{k}={r.get(k, '?')}" for _, k in FIELDS))
    return 0


if __name__ == "__main__":
    sys.exit(main())
