"""Registers, LDS, scratch and a hash of the machine code of every kernel of a
source tree, one line per kernel symbol (device code only, no GPU needed): the
resources from hipcc's -Rpass-analysis=kernel-resource-usage, the hash over the
kernel's function bytes in the gfx950 ELF of the same compile.  Two trees side
by side show whether a change touched the code of kernels it did not mean to:

    python tools/kernel_resources.py                       # this tree
    python tools/kernel_resources.py --root /path/to/other/checkout
    python tools/kernel_resources.py --against /path/to/other/checkout   # one line per kernel, both sides

--against matches kernels by name, whichever file defines them, and exits 1
when a kernel is missing on one side or differs in hash or resources.
"""
import argparse
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
FIELDS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("ScratchSize [bytes/lane]", "scratch"),
          ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds"))
READELF = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf")


def code_hashes(obj):
    """{symbol: sha256 of its bytes} for the FUNC symbols of the ELF's .text."""
    out = subprocess.run([READELF, "-S", "-s", "--wide", obj], check=True, capture_output=True, text=True).stdout
    m = re.search(r"\]\s+\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", out)
    addr, off, size = (int(x, 16) for x in m.groups())
    with open(obj, "rb") as f:
        blob = f.read()
    hashes = {}
    for m in re.finditer(r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\d+\s+(\S+)$", out, re.M):
        value, n, name = int(m.group(1), 16), int(m.group(2)), m.group(3)
        assert addr <= value and value + n <= addr + size, name
        hashes[name] = hashlib.sha256(blob[off + value - addr:off + value - addr + n]).hexdigest()[:16]
    return hashes


def resources(src, root, arch):
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "dev.o")
        cmd = ["hipcc", "-x", "hip", f"--offload-arch={arch}", "--cuda-device-only", "--no-gpu-bundle-output", "-O3",
               "-std=c++17", "-Rpass-analysis=kernel-resource-usage", "-Wno-unused-function", "-I",
               os.path.join(root, "include"), "-I", os.path.dirname(src), "-c", src, "-o", obj]
        err = subprocess.run(cmd, check=True, capture_output=True, text=True).stderr
        hashes = code_hashes(obj)
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {"hash": hashes.get(m.group(1), "?")})
            continue
        for label, key in FIELDS:
            m = re.search(r"remark:\s+" + re.escape(label) + r": (\d+)", line)
            if m and cur is not None:
                cur[key] = int(m.group(1))
    return out


def tree(root, arch):
    """[(file, demangled kernel, fields)] of every .hip under root's csrc, sorted."""
    srcs = sorted(glob.glob(os.path.join(root, "kuma_amd", "csrc", "*.hip")))
    with ThreadPoolExecutor(max_workers=4) as ex:
        per = list(ex.map(lambda s: resources(s, root, arch), srcs))
    rows = []
    for src, res in zip(srcs, per):
        for name in sorted(res):
            sym = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
            rows.append((os.path.basename(src), sym, res[name]))
    return rows


def fields(r):
    return "  ".join(f"{k}={r.get(k, '?')}" for _, k in FIELDS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--against", help="another checkout: one line per kernel with both sides")
    ap.add_argument("--arch", default="gfx950")
    a = ap.parse_args()
    rows = tree(a.root, a.arch)
    if not a.against:
        for f, sym, r in rows:
            print(f"{f}  {sym}  hash={r['hash']}  {fields(r)}")
        return 0
    mine = {sym: (f, r) for f, sym, r in rows}
    theirs = {sym: (f, r) for f, sym, r in tree(a.against, a.arch)}
    differ = 0
    for sym in sorted(set(mine) | set(theirs)):
        (f0, r0), (f1, r1) = theirs.get(sym, ("-", {})), mine.get(sym, ("-", {}))
        same = r0 == r1 and bool(r0)
        differ += not same
        print(f"{'same' if same else 'DIFF'}  {sym}  other: {f0} hash={r0.get('hash', '-')} {fields(r0)}  "
              f"this: {f1} hash={r1.get('hash', '-')} {fields(r1)}")
    print(f"# {len(mine)} kernels here, {len(theirs)} there, {differ} lines differ")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
