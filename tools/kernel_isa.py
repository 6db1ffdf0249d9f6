#!/usr/bin/env python3
"""SHA-256 of the gfx950 assembly hipcc emits for some csrc/*.hip files (device pass only, the Makefile's flags, -S; needs
no GPU, seconds per file).  Two source trees whose digests are equal ship the same device code: a refactor that only
moves or renames source text is proven by running this on both.  Lines that hold the per-compile unique id
(__hip_cuid_...) are dropped; they are the only ones that differ between two compiles of equivalent source.  Prints
one JSON object {file: digest}:
    python tools/kernel_isa.py [--csrc DIR] [-j N] gemm_split.hip conv3x3.hip ...
"""
import argparse
import hashlib
import json
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
         "--cuda-device-only", "-S", "-o", "-"]


def assembly(csrc, name, hipcc="/opt/rocm/bin/hipcc"):
    """The device assembly of csrc/name, compiled from inside csrc so that no directory name gets into it."""
    run = subprocess.run([hipcc] + FLAGS + ["-x", "hip", name], cwd=csrc, capture_output=True, text=True)
    if run.returncode:
        raise SystemExit(f"{name} does not compile:\n{run.stderr}")
    out = run.stdout
    return "".join(l for l in out.splitlines(keepends=True) if "__hip_cuid_" not in l)


def digest(csrc, name):
    return hashlib.sha256(assembly(csrc, name).encode()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(os.path.dirname(HERE), "racformer_amd", "csrc"))
    ap.add_argument("-j", type=int, default=4, help="compiles in flight")
    ap.add_argument("--dump", help="also write each file's filtered assembly as DIR/<file>.s")
    ap.add_argument("files", nargs="+")
    args = ap.parse_args()
    with ThreadPoolExecutor(args.j) as pool:
        asm = dict(zip(args.files, pool.map(lambda f: assembly(args.csrc, f), args.files)))
    if args.dump:
        os.makedirs(args.dump, exist_ok=True)
        for f, text in asm.items():
            with open(os.path.join(args.dump, f + ".s"), "w") as fh:
                fh.write(text)
    print(json.dumps({f: hashlib.sha256(text.encode()).hexdigest() for f, text in asm.items()}, indent=1))


if __name__ == "__main__":
    main()
