#!/usr/bin/env python3
"""Device-event times of the AdaptiveMixing core's forward and backward at the f8 shape (B = 1, Q = 900, G = 4 groups of 64
channels, P = 96 in points, 128 out points, fp32; x [1,900,4,96,64] = 88 MB, params [1,900,4*(4096+128*96)] = 236 MB):
  rac_mixing_fwd F32      the training forward (RAC_MIX_F32)
  rac_mixing_bwd          dx and [dM | dS] from x, params and dZ (the forward recomputed on chip)
  torch backward          the autograd backward of the unfused core (two batched matmuls, two LayerNorms, two ReLUs),
                          its graph built once and replayed
  torch backward + recompute   that backward after re-running the core's forward, as the reference's gradient
                          checkpointing does (models/racformer_transformer.py:612-616)
After a warm-up the two sides of a pair run in alternating batches of launches, each batch between two events, until each
has at least --window-ms of timed launches; reported per launch: median and mean over the batches.

    python tools/mixing_bwd_timing.py [--out profiles/mixing_bwd_f8.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from msmv_v2_timing import summary, time_pair  # noqa: E402
from racformer_amd.fused import mixing_backward, mixing_fused  # noqa: E402


def torch_core(x, params, P, G):
    """AdaptiveMixing.forward's torch path up to out_proj (racformer_transformer.py:589-603)"""
    B, Q = x.shape[:2]
    p = params.reshape(B * Q, G, -1)
    M, S = p.split([64 * 64, 128 * P], 2)
    out = torch.matmul(x.reshape(B * Q, G, P, 64), M.reshape(B * Q, G, 64, 64))
    out = F.relu(F.layer_norm(out, [out.size(-2), out.size(-1)]))
    out = torch.matmul(S.reshape(B * Q, G, 128, P), out)
    out = F.relu(F.layer_norm(out, [out.size(-2), out.size(-1)]))
    return out.reshape(B, Q, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda:0"
    B, Q, G, P = 1, 900, 4, 96
    W = G * (64 * 64 + 128 * P)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, Q, G, P, 64, generator=g).to(dev)
    params = (torch.randn(B, Q, W, generator=g) * 0.1).to(dev)
    gout = torch.randn(B, Q, G * 128 * 64, generator=g).to(dev)
    gx, gp = torch.empty_like(x), torch.empty_like(params)
    out = mixing_fused(x, params, P, G, f16x3=False)

    def fwd():
        mixing_fused(x, params, P, G, f16x3=False)

    def bwd():
        mixing_backward(x, params, gout, P, G, grad_x=gx, grad_params=gp)

    xt, pt = x.clone().requires_grad_(), params.clone().requires_grad_()
    o_t = torch_core(xt, pt, P, G)
    assert (o_t.detach() - out).abs().max().item() < 1e-3
    ref = torch.autograd.grad(o_t, [xt, pt], gout, retain_graph=True)
    bwd()
    torch.cuda.synchronize()
    rel = {k: ((a - b).abs().max() / b.abs().max()).item() for k, a, b in (("dx", gx, ref[0]), ("dparams", gp, ref[1]))}

    def torch_bwd():
        torch.autograd.grad(o_t, [xt, pt], gout, retain_graph=True)

    def torch_ckpt():
        xr, pr = x.detach().requires_grad_(), params.detach().requires_grad_()
        torch.autograd.grad(torch_core(xr, pr, P, G), [xr, pr], gout)

    rec = {"what": "AdaptiveMixing core at f8: rac_mixing_fwd (F32), rac_mixing_bwd, and the torch autograd backward of the "
                   "unfused core, without and with the recompute of gradient checkpointing; alternating batches of launches "
                   "between device events (tools/mixing_bwd_timing.py)",
           "shape": {"B": B, "Q": Q, "G": G, "P": P, "channels": 64, "out_points": 128, "dtype": "float32"},
           "batch": args.batch, "warmup_launches_each": args.warmup, "device": torch.cuda.get_device_name(0),
           "bytes_moved_bwd_MB": round((x.numel() * 2 + params.numel() * 2 + gout.numel()) * 4 / 1e6, 1),
           "bwd_vs_torch_fp32_max_rel_diff": {k: float(f"{v:.3g}") for k, v in rel.items()}}
    res, total = time_pair(fwd, bwd, args.batch, args.window_ms, args.warmup)
    rec["rac_mixing_fwd_f32"], rec["rac_mixing_bwd"] = summary(res["a"], total["a"]), summary(res["b"], total["b"])
    res, total = time_pair(torch_bwd, torch_ckpt, args.batch, args.window_ms, args.warmup)
    rec["torch_unfused_core_backward"], rec["torch_unfused_core_recompute_and_backward"] = (summary(res["a"], total["a"]),
                                                                                            summary(res["b"], total["b"]))
    bw = rec["rac_mixing_bwd"]["median_us"]
    rec["bwd_over_fwd_median"] = round(bw / rec["rac_mixing_fwd_f32"]["median_us"], 2)
    rec["torch_bwd_over_bwd_median"] = round(rec["torch_unfused_core_backward"]["median_us"] / bw, 2)
    rec["torch_recompute_bwd_over_bwd_median"] = round(rec["torch_unfused_core_recompute_and_backward"]["median_us"] / bw, 2)
    rec["bwd_effective_TBps"] = round(rec["bytes_moved_bwd_MB"] * 1e6 / (bw * 1e-6) / 1e12, 2)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
