#!/usr/bin/env python3
"""Register, LDS and scratch figures of every __global__ kernel of some csrc/*.hip files, as hipcc reports them
(-Rpass-analysis=kernel-resource-usage, device pass only, the Makefile's flags; needs no GPU).  Prints one JSON object
{file: {demangled kernel: {vgprs, agprs, scratch, occupancy, lds}}}:
    python tools/kernel_resources.py [--csrc DIR] resnet.hip resnet_bwd.hip ...
"""
import argparse
import json
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
         "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o", os.devnull]
KEYS = {"VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy",
        "LDS Size [bytes/block]": "lds"}


def resources(path, hipcc="/opt/rocm/bin/hipcc"):
    err = subprocess.run([hipcc] + FLAGS + [path], check=True, capture_output=True, text=True).stderr
    out, cur = {}, None
    for line in err.splitlines():
        m = re.search(r"remark: +([A-Za-z\[\]/ ]+?): (\S+) \[-Rpass-analysis", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = subprocess.run(["c++filt", m.group(2)], capture_output=True, text=True).stdout.strip()
            cur = out.setdefault(re.sub(r"\(.*\)$", "", name).replace("void ", ""), {})
        elif cur is not None and m.group(1) in KEYS:
            cur[KEYS[m.group(1)]] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(os.path.dirname(HERE), "racformer_amd", "csrc"))
    ap.add_argument("files", nargs="+")
    args = ap.parse_args()
    print(json.dumps({f: resources(os.path.join(args.csrc, f)) for f in args.files}, indent=1))


if __name__ == "__main__":
    main()
