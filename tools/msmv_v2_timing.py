#!/usr/bin/env python3
"""Device-event times of rac_msmv_v2_fwd / rac_msmv_v2_bwd next to rac_msmv_fwd / rac_msmv_bwd on the same f8-shaped inputs
(S = 32 slots, N = 6 cameras, Q = 900, P = 12, C = 64, the four f8 pyramid levels, fp32, tests/test_msmv_v2_gpu.py's
f8 case).  After a warm-up the two kernels of a pair run in alternating batches of launches, each batch between two events,
until every kernel has at least --window-ms of timed launches; reported per launch: median and mean over the batches.
The backward buffers are not re-zeroed between launches (the adds just accumulate): the times are of the kernels alone.

    python tools/msmv_v2_timing.py [--out profiles/msmv_v2_f8.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from racformer_amd import _lib, synthetic as syn  # noqa: E402


def f8_case(dev):
    S, N, Q, P, C = 32, 6, 900, 12, 64
    rng = np.random.default_rng(0)
    feats = [torch.from_numpy(syn.smooth_noise(70 + i, (S, N), h, w * C).reshape(S, N, h, w, C)).to(dev)
             for i, (h, w) in enumerate(syn.F8.fpn_hw)]
    loc = rng.random((S, Q, P, 3), dtype=np.float32) * 1.1 - 0.05
    loc[..., 2] = rng.integers(0, N, size=(S, Q, P)).astype(np.float32) / np.float32(N - 1)
    w = rng.standard_normal((S, Q, P, 4), dtype=np.float32)
    w = np.exp(w) / np.exp(w).sum(-1, keepdims=True)
    return feats, torch.from_numpy(loc).to(dev), torch.from_numpy(w.astype(np.float32)).to(dev), (S, N, Q, P, C)


def time_pair(launch_a, launch_b, batch, window_ms, warmup):
    """alternating batches of `batch` launches of a and b, each batch between two events -> per-launch ms lists"""
    for _ in range(warmup):
        launch_a()
        launch_b()
    torch.cuda.synchronize()
    res = {"a": [], "b": []}
    total = {"a": 0.0, "b": 0.0}
    while min(total.values()) < window_ms:
        for key, fn in (("a", launch_a), ("b", launch_b)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1)
            total[key] += ms
            res[key].append(ms / batch)
    return res, total


def summary(per_launch, total_ms):
    return {"median_us": round(statistics.median(per_launch) * 1e3, 2), "mean_us": round(statistics.mean(per_launch) * 1e3, 2),
            "min_us": round(min(per_launch) * 1e3, 2), "batches": len(per_launch), "timed_ms": round(total_ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda:0"
    lib = _lib.lib()
    feats, loc, w, (S, N, Q, P, C) = f8_case(dev)
    L = len(feats)
    ptrs = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats])
    hw = (ctypes.c_int32 * (2 * L))(*[int(x) for f in feats for x in f.shape[2:4]])
    out = torch.empty(S, Q, C, P, device=dev)
    gout = torch.from_numpy(np.random.default_rng(1).standard_normal((S, Q, C, P), dtype=np.float32)).to(dev)
    gfeat = [torch.zeros_like(f) for f in feats]
    gptrs = (ctypes.c_void_p * L)(*[g.data_ptr() for g in gfeat])
    gloc = torch.empty_like(loc)
    gw = torch.empty_like(w)
    st = _lib.stream_ptr()
    P_ = _lib.ptr

    def v1_fwd():
        _lib.check(lib.rac_msmv_fwd(ptrs, hw, L, P_(loc), P_(w), P_(out), S, N, Q, P, C, _lib.RAC_F32, _lib.OUT_SQCP, 1, 1, st),
                   "rac_msmv_fwd")

    def v2_fwd():
        _lib.check(lib.rac_msmv_v2_fwd(ptrs, hw, L, P_(loc), P_(w), P_(out), S, N, Q, P, C, _lib.RAC_F32, _lib.FEAT_CL,
                                       _lib.OUT_SQCP, 1, 1, st), "rac_msmv_v2_fwd")

    def v1_bwd():
        _lib.check(lib.rac_msmv_bwd(P_(gout), ptrs, hw, L, P_(loc), P_(w), gptrs, P_(gloc), P_(gw), S, N, Q, P, C, st),
                   "rac_msmv_bwd")

    def v2_bwd():
        _lib.check(lib.rac_msmv_v2_bwd(P_(gout), ptrs, hw, L, P_(loc), P_(w), gptrs, P_(gloc), S, N, Q, P, C, _lib.FEAT_CL, st),
                   "rac_msmv_v2_bwd")

    rec = {"what": "rac_msmv_v2_{fwd,bwd} against rac_msmv_{fwd,bwd}, same inputs, alternating batches of launches between "
                   "device events (tools/msmv_v2_timing.py)",
           "shape": {"S": S, "N": N, "Q": Q, "P": P, "C": C, "levels_hw": [list(f.shape[2:4]) for f in feats], "dtype": "float32",
                     "out_layout": "SQCP"},
           "batch": args.batch, "warmup_launches_each": args.warmup, "device": torch.cuda.get_device_name(0)}
    for name, (a, b) in (("forward", (v1_fwd, v2_fwd)), ("backward", (v1_bwd, v2_bwd))):
        res, total = time_pair(a, b, args.batch, args.window_ms, args.warmup)
        v1, v2 = summary(res["a"], total["a"]), summary(res["b"], total["b"])
        rec[name] = {"rac_msmv": v1, "rac_msmv_v2": v2, "v2_over_v1_median": round(v2["median_us"] / v1["median_us"], 3)}
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
