#!/usr/bin/env python3
"""Device-event times of the masked SASA core at the query-denoising shapes (B = 1, 8 heads of 32, fp32, the lin operand a
[1,Q,776] in_proj + gen_tau output, centres from the box table; the mask: 10 denoising groups in front of 900 matching queries,
Q = 1300 (40 boxes) and Q = 1700 (80 boxes)):
  rac_sasa_fwd_mask     the masked forward writing each row's log-sum-exp (the streaming matrix-core kernel at these Q)
  rac_sasa_bwd_mask     dq, dk, dv, dtau under the mask
  torch fwd + bwd       forward_unfused's core (cdist mask, indexed -inf fill, QK^T, softmax, AV on [1,8,Q,Q]) and its autograd
                        backward: the route a masked call took before the masked kernels existed
After a warm-up the two sides of a pair run in alternating batches of launches, each batch between two events, until each has
at least --window-ms of timed launches; reported per launch: median, mean and minimum over the batches.  Peak memory
(torch.cuda.max_memory_allocated over one forward + backward, above what was allocated before it) is recorded for both routes.

    python tools/sasa_mask_timing.py [--out profiles/sasa_mask_f8.json]
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
from racformer_amd.fused import box_prep, pack_attn_mask, sasa_backward, sasa_fused  # noqa: E402


def dn_mask(groups, single, matching, device):
    pad = groups * single
    idx = torch.arange(pad + matching, device=device)
    group = torch.where(idx < pad, torch.div(idx, single, rounding_mode="floor"), torch.full_like(idx, -1))
    return (idx[None, :] < pad) & (group[:, None] != group[None, :])


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)


def one_shape(single, args):
    dev = "cuda:0"
    B, H, d, groups, matching = 1, 8, 32, 10, 900
    Q, E = groups * single + matching, H * d
    g = torch.Generator().manual_seed(single)
    lin = torch.randn(B, Q, 3 * E + H, generator=g).to(dev)
    lin[..., 3 * E:] = torch.rand(B, Q, H, generator=g).to(dev) * 2
    qb = torch.rand(B, Q, 10, generator=g).to(dev)
    gout = torch.randn(B, Q, E, generator=g).to(dev)
    table = box_prep(qb, syn.PC_RANGE)
    mask = dn_mask(groups, single, matching, dev)
    pk = pack_attn_mask(mask)
    qkv, tau = lin[..., :3 * E], lin[..., 3 * E:]
    lse = torch.empty(B, H, Q, device=dev)
    out = sasa_fused(qkv, tau, qb, H, syn.PC_RANGE, box_table=table, lse_out=lse, mask=pk)
    grad_lin = torch.empty_like(lin)

    def fwd():
        sasa_fused(qkv, tau, qb, H, syn.PC_RANGE, box_table=table, lse_out=lse, mask=pk)

    def bwd():
        sasa_backward(qkv, tau, qb, H, syn.PC_RANGE, out, lse, gout, box_table=table, grad_qkv=grad_lin[..., :3 * E],
                      grad_tau=grad_lin[..., 3 * E:], mask=pk)

    def fused_step():
        fwd()
        bwd()

    # forward_unfused's core on the same operands: a fresh graph per step (the [B,8,Q,Q] mask and probabilities are per step)
    centers = decode_bbox(theta_d2xy_coods(qb), syn.PC_RANGE)[..., :2]

    def torch_forward(lt):
        dist = -torch.cdist(centers, centers, compute_mode="donot_use_mm_for_euclid_dist")
        m = dist[:, None] * lt[..., 3 * E:].permute(0, 2, 1)[..., None]
        m[:, :, mask] = float("-inf")
        x = lt[..., :3 * E].view(B, Q, 3, H, d)
        q = x[:, :, 0].permute(0, 2, 1, 3) * math.sqrt(1.0 / d)
        k = x[:, :, 1].permute(0, 2, 1, 3)
        v = x[:, :, 2].permute(0, 2, 1, 3)
        return (torch.softmax(m + q @ k.transpose(-1, -2), dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, Q, E)

    lt = lin.clone().requires_grad_()
    assert (torch_forward(lt).detach() - out).abs().max().item() < 1e-4

    def torch_fwd():
        with torch.no_grad():
            torch_forward(lin)

    def torch_step():
        torch.autograd.grad(torch_forward(lt), [lt], gout)

    rec = {"shape": {"B": B, "Q": Q, "heads": H, "head_dim": d, "groups": groups, "boxes": single, "ld_lin": 3 * E + H,
                     "box_table": True, "dtype": "float32", "blocked_fraction": round(float(mask.float().mean()), 4)}}
    res, total = time_pair(fwd, torch_fwd, args.batch, args.window_ms, args.warmup)
    rec["rac_sasa_fwd_mask"], rec["torch_unfused_core_forward"] = summary(res["a"], total["a"]), summary(res["b"], total["b"])
    res, total = time_pair(fused_step, torch_step, args.batch, args.window_ms, args.warmup)
    rec["fused_forward_plus_backward"], rec["torch_unfused_forward_plus_backward"] = summary(res["a"], total["a"]), summary(res["b"], total["b"])
    res, total = time_pair(bwd, fwd, args.batch, args.window_ms, args.warmup)
    rec["rac_sasa_bwd_mask"] = summary(res["a"], total["a"])
    rec["peak_mb_fused_forward_plus_backward"] = peak_mb(fused_step)
    rec["peak_mb_torch_forward_plus_backward"] = peak_mb(torch_step)
    rec["torch_over_fused_step_median"] = round(rec["torch_unfused_forward_plus_backward"]["median_us"] / rec["fused_forward_plus_backward"]["median_us"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--window-ms", type=float, default=400.0)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rec = {"what": "masked SASA core at the query-denoising shapes: rac_sasa_fwd_mask (lse written), rac_sasa_bwd_mask, their sum, and "
                   "forward_unfused's core with torch autograd; alternating batches of launches between device events "
                   "(tools/sasa_mask_timing.py)",
           "batch": args.batch, "warmup_launches_each": args.warmup, "window_ms": args.window_ms,
           "device": torch.cuda.get_device_name(0)}
    for single in (40, 80):
        rec[f"Q{10 * single + 900}"] = one_shape(single, args)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
