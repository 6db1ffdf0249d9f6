#!/usr/bin/env python3
"""A/B of rac_mixing_fwd between builds of libracformer_hip.so, in one process: the inference call of AdaptiveMixing.forward
(RAC_MIX_F16X3, the f16 split image as output) at the f8 shape -- Q = 900, G = 4 groups of 64 channels, P = 96 in points, 128 out
points: x 88 MB, params 236 MB, image 118 MB per launch.

Every build is loaded side by side (ctypes; a build named twice is copied first, so that it is loaded as a library of its own
and its second figure is the run-to-run spread of identical code).  After a warm-up the builds take turns, one batch of launches
each between two device events, for --rounds rounds; reported per build: median, mean, min and max over its batches, per launch.
The outputs of the builds on the same inputs are compared too (identical bits, or the largest difference).

    python tools/mixing_fwd_ab.py --lib parent=build/parent.so --lib parent_again=build/parent.so --lib new=racformer_amd/csrc/libracformer_hip.so \\
        [--out profiles/mixing_fwd_s_scale_ab.json]
"""
import argparse
import ctypes
import json
import os
import shutil
import statistics
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from racformer_amd import _lib  # noqa: E402
from racformer_amd.fused import SPLIT_ACT_SCALE  # noqa: E402


def load(path):
    handle = ctypes.CDLL(path)
    for name in ("rac_mixing_fwd", "rac_last_error"):
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return handle


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", required=True, help="name=path, at least two")
    ap.add_argument("--out", default="")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--s-std", type=float, default=0.1)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    named = [a.split("=", 1) for a in args.lib]
    assert len(named) >= 2 and len({n for n, _ in named}) == len(named)
    tmp = tempfile.mkdtemp(prefix="mixing_ab_")
    libs, seen = {}, set()
    for name, path in named:
        path = os.path.abspath(path)
        if path in seen:                               # the same file again: a copy, loaded as a library of its own
            copy = os.path.join(tmp, f"{name}.so")
            shutil.copy(path, copy)
            path = copy
        seen.add(path)
        libs[name] = load(path)

    dev = "cuda:0"
    Q, G, P = 900, 4, 96
    width = G * (64 * 64 + 128 * P)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(1, Q, G, P, 64, generator=g, device=dev)
    params = torch.randn(1, Q, width, generator=g, device=dev) * args.s_std
    outs = {n: torch.empty(Q, G * 256, 64, device=dev, dtype=torch.float16) for n in libs}
    stream = _lib.stream_ptr()

    def launch(name):
        rc = libs[name].rac_mixing_fwd(_lib.ptr(x), _lib.ptr(params), 1.0, None, _lib.ptr(outs[name]), SPLIT_ACT_SCALE, width, Q, G, P, 64,
                                       128, 1e-5, _lib.MIX_F16X3, stream)
        if rc != 0:
            raise RuntimeError(f"{name}: rac_mixing_fwd failed (rc={rc}): {libs[name].rac_last_error().decode(errors='replace')}")

    for name in libs:
        for _ in range(args.warmup):
            launch(name)
    torch.cuda.synchronize()
    first = next(iter(libs))
    img = {n: o.float().view(Q, G * 256, 2, 32) for n, o in outs.items()}
    val = {n: ((i[:, :, 0] + i[:, :, 1]) / SPLIT_ACT_SCALE) for n, i in img.items()}
    same = {n: dict(bit_identical_to_first=bool(torch.equal(outs[n], outs[first])),
                    max_abs_diff_to_first=float((val[n] - val[first]).abs().max()), max_abs_value=float(val[n].abs().max()))
            for n in libs if n != first}
    del img, val

    events = {n: [] for n in libs}
    for _ in range(args.rounds):
        for name in libs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.batch):
                launch(name)
            e1.record()
            events[name].append((e0, e1))
    torch.cuda.synchronize()
    rec = {"what": "rac_mixing_fwd (RAC_MIX_F16X3, split image out) at f8, builds of the library taking turns in one process, one batch of "
                   "launches each between two device events (tools/mixing_fwd_ab.py); us per launch over the batches",
           "shape": {"Q": Q, "G": G, "P": P, "channels": 64, "out_points": 128, "std_S": args.s_std},
           "batch": args.batch, "rounds": args.rounds, "warmup_launches_each": args.warmup, "device": torch.cuda.get_device_name(0),
           "builds": {}, "outputs_against_first": same}
    for name, evs in events.items():
        us = [e0.elapsed_time(e1) * 1e3 / args.batch for e0, e1 in evs]
        rec["builds"][name] = {"median_us": round(statistics.median(us), 2), "mean_us": round(statistics.fmean(us), 2),
                               "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                               "p10_us": round(sorted(us)[len(us) // 10], 2), "p90_us": round(sorted(us)[len(us) * 9 // 10], 2)}
    shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
