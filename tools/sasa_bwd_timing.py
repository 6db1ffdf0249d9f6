#!/usr/bin/env python3
"""Device-event times of the SASA core's forward and backward at the f8 shape (B = 1, Q = 900, 8 heads of 32, fp32, the lin
operand a [1,900,776] in_proj + gen_tau output, centres from the box table as the decoder layer passes them):
  rac_sasa_fwd          the inference forward (what the benchmark runs)
  rac_sasa_fwd_ex       the same forward writing each row's log-sum-exp (the training forward)
  rac_sasa_bwd          dq, dk, dv, dtau from the saved output and lse
  torch backward        the autograd backward of forward_unfused's core (cdist mask, QK^T, softmax, AV on [1,8,900,900])
After a warm-up the two sides of a pair run in alternating batches of launches, each batch between two events, until each
has at least --window-ms of timed launches; reported per launch: median and mean over the batches.

    python tools/sasa_bwd_timing.py [--out profiles/sasa_bwd_f8.json]
"""
import argparse
import json
import math
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from msmv_v2_timing import summary, time_pair  # noqa: E402
from racformer_amd import synthetic as syn  # noqa: E402
from racformer_amd.bbox_utils import decode_bbox, theta_d2xy_coods  # noqa: E402
from racformer_amd.fused import box_prep, sasa_backward, sasa_fused  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--batch", type=int, default=20)
    ap.add_argument("--window-ms", type=float, default=250.0)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda:0"
    B, Q, H, d = 1, 900, 8, 32
    E = H * d
    g = torch.Generator().manual_seed(0)
    lin = torch.randn(B, Q, 3 * E + H, generator=g).to(dev)
    lin[..., 3 * E:] = torch.rand(B, Q, H, generator=g).to(dev) * 2
    qb = torch.rand(B, Q, 10, generator=g).to(dev)
    gout = torch.randn(B, Q, E, generator=g).to(dev)
    table = box_prep(qb, syn.PC_RANGE)
    qkv, tau = lin[..., :3 * E], lin[..., 3 * E:]
    lse = torch.empty(B, H, Q, device=dev)
    out = sasa_fused(qkv, tau, qb, H, syn.PC_RANGE, box_table=table, lse_out=lse)
    grad_lin = torch.empty_like(lin)

    def fwd():
        sasa_fused(qkv, tau, qb, H, syn.PC_RANGE, box_table=table)

    def fwd_ex():
        sasa_fused(qkv, tau, qb, H, syn.PC_RANGE, box_table=table, lse_out=lse)

    def bwd():
        sasa_backward(qkv, tau, qb, H, syn.PC_RANGE, out, lse, gout, box_table=table, grad_qkv=grad_lin[..., :3 * E],
                      grad_tau=grad_lin[..., 3 * E:])

    # forward_unfused's core on the same operands, its graph built once and its backward replayed
    lt = lin.clone().requires_grad_()
    centers = decode_bbox(theta_d2xy_coods(qb), syn.PC_RANGE)[..., :2]
    dist = -torch.cdist(centers, centers, compute_mode="donot_use_mm_for_euclid_dist")
    t_ = lt[..., 3 * E:].permute(0, 2, 1)
    x = lt[..., :3 * E].view(B, Q, 3, H, d)
    q = x[:, :, 0].permute(0, 2, 1, 3) * math.sqrt(1.0 / d)
    k = x[:, :, 1].permute(0, 2, 1, 3)
    v = x[:, :, 2].permute(0, 2, 1, 3)
    o_t = (torch.softmax(dist[:, None] * t_[..., None] + q @ k.transpose(-1, -2), dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, Q, E)
    assert (o_t.detach() - out).abs().max().item() < 1e-4

    def torch_bwd():
        torch.autograd.grad(o_t, [lt], gout, retain_graph=True)

    rec = {"what": "SASA core at f8: rac_sasa_fwd, rac_sasa_fwd_ex (lse written), rac_sasa_bwd, and the torch autograd backward "
                   "of forward_unfused's core; alternating batches of launches between device events (tools/sasa_bwd_timing.py)",
           "shape": {"B": B, "Q": Q, "heads": H, "head_dim": d, "ld_lin": 3 * E + H, "box_table": True, "dtype": "float32"},
           "batch": args.batch, "warmup_launches_each": args.warmup, "device": torch.cuda.get_device_name(0)}
    res, total = time_pair(fwd, fwd_ex, args.batch, args.window_ms, args.warmup)
    rec["rac_sasa_fwd"], rec["rac_sasa_fwd_ex_lse"] = summary(res["a"], total["a"]), summary(res["b"], total["b"])
    res, total = time_pair(bwd, torch_bwd, args.batch, args.window_ms, args.warmup)
    rec["rac_sasa_bwd"], rec["torch_unfused_core_backward"] = summary(res["a"], total["a"]), summary(res["b"], total["b"])
    rec["bwd_over_fwd_median"] = round(rec["rac_sasa_bwd"]["median_us"] / rec["rac_sasa_fwd"]["median_us"], 2)
    rec["torch_bwd_over_bwd_median"] = round(rec["torch_unfused_core_backward"]["median_us"] / rec["rac_sasa_bwd"]["median_us"], 2)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
