#!/usr/bin/env python3
"""Device-event times of sampling_4d's backward with the gradient read directly in the forward's [B,Q,G,T*P,C] layout
(rac_msmv_bwd_ex / rac_msmv_v2_bwd_ex, RAC_OUT_BQGTPC) against what a plain autograd wrapper would do: permute-copy the
gradient to [S,Q,C,P] and run rac_msmv_bwd / rac_msmv_v2_bwd.  f8 shape (B = 1, T = 8, G = 4: S = 32 slots, N = 6 cameras,
Q = 900, P = 12, C = 64, the four f8 pyramid levels, fp32; the inputs of tools/msmv_v2_timing.py).  After a warm-up the two
sides of a pair run in alternating batches of launches, each batch between two events, until each has at least
--window-ms of timed launches; reported per launch: median and mean over the batches.  Also timed: the SQCP kernel alone
(gradient already in [S,Q,C,P]) against the BQGTPC kernel, and the permute copy alone.  The feature-gradient buffers are
not re-zeroed between launches (the adds just accumulate): the times are of the kernels (and the copy) alone.

    python tools/sampling4d_bwd_timing.py [--out profiles/sampling4d_bwd_f8.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from racformer_amd import _lib  # noqa: E402
from msmv_v2_timing import f8_case, summary, time_pair  # noqa: E402


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
    B, T, G = 1, 8, 4
    assert B * T * G == S
    L = len(feats)
    ptrs = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats])
    hw = (ctypes.c_int32 * (2 * L))(*[int(x) for f in feats for x in f.shape[2:4]])
    g_bq = torch.from_numpy(np.random.default_rng(1).standard_normal((B, Q, G, T * P, C), dtype=np.float32)).to(dev)
    g_sq = torch.empty(S, Q, C, P, device=dev)
    sq_view = g_bq.view(B, Q, G, T, P, C).permute(0, 3, 2, 1, 5, 4).reshape(S, Q, C, P)   # (a view: no copy yet)
    g_sq.copy_(sq_view)
    gfeat = [torch.zeros_like(f) for f in feats]
    gptrs = (ctypes.c_void_p * L)(*[g.data_ptr() for g in gfeat])
    gloc = torch.empty_like(loc)
    gw = torch.empty_like(w)
    st = _lib.stream_ptr()
    P_ = _lib.ptr

    def v1_bq():
        _lib.check(lib.rac_msmv_bwd_ex(P_(g_bq), _lib.OUT_BQGTPC, T, G, ptrs, hw, L, P_(loc), P_(w), gptrs, P_(gloc), P_(gw),
                                       S, N, Q, P, C, st), "rac_msmv_bwd_ex")

    def v1_sq():
        _lib.check(lib.rac_msmv_bwd(P_(g_sq), ptrs, hw, L, P_(loc), P_(w), gptrs, P_(gloc), P_(gw), S, N, Q, P, C, st),
                   "rac_msmv_bwd")

    def v2_bq():
        _lib.check(lib.rac_msmv_v2_bwd_ex(P_(g_bq), _lib.OUT_BQGTPC, T, G, ptrs, hw, L, P_(loc), P_(w), gptrs, P_(gloc),
                                          S, N, Q, P, C, _lib.FEAT_CL, st), "rac_msmv_v2_bwd_ex")

    def v2_sq():
        _lib.check(lib.rac_msmv_v2_bwd(P_(g_sq), ptrs, hw, L, P_(loc), P_(w), gptrs, P_(gloc), S, N, Q, P, C, _lib.FEAT_CL, st),
                   "rac_msmv_v2_bwd")

    def permute():
        g_sq.copy_(sq_view)

    rec = {"what": "sampling_4d backward: gradient read in [B,Q,G,T*P,C] (rac_msmv_bwd_ex / rac_msmv_v2_bwd_ex, RAC_OUT_BQGTPC) "
                   "against permute-copy to [S,Q,C,P] + rac_msmv_bwd / rac_msmv_v2_bwd; alternating batches of launches "
                   "between device events (tools/sampling4d_bwd_timing.py)",
           "shape": {"B": B, "T": T, "G": G, "S": S, "N": N, "Q": Q, "P": P, "C": C,
                     "levels_hw": [list(f.shape[2:4]) for f in feats], "dtype": "float32",
                     "gradient_mb": round(g_bq.numel() * 4 / 1e6, 1)},
           "batch": args.batch, "warmup_launches_each": args.warmup, "device": torch.cuda.get_device_name(0)}
    for name, a, b in (("rac_msmv_bwd", v1_bq, lambda: (permute(), v1_sq())), ("rac_msmv_v2_bwd", v2_bq, lambda: (permute(), v2_sq()))):
        res, total = time_pair(a, b, args.batch, args.window_ms, args.warmup)
        direct, copied = summary(res["a"], total["a"]), summary(res["b"], total["b"])
        res2, total2 = time_pair(a, v1_sq if name == "rac_msmv_bwd" else v2_sq, args.batch, args.window_ms, args.warmup)
        k_bq, k_sq = summary(res2["a"], total2["a"]), summary(res2["b"], total2["b"])
        rec[name] = {"direct_bqgtpc": direct, "permute_copy_plus_sqcp": copied,
                     "direct_over_permute_median": round(direct["median_us"] / copied["median_us"], 3),
                     "kernel_only": {"bqgtpc": k_bq, "sqcp": k_sq,
                                     "bqgtpc_over_sqcp_median": round(k_bq["median_us"] / k_sq["median_us"], 3)}}
    res, total = time_pair(permute, permute, args.batch, args.window_ms, args.warmup)
    rec["permute_copy_alone"] = summary(res["a"] + res["b"], total["a"] + total["b"])
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
