#!/usr/bin/env python3
"""Time rac_sampling4d_bwd at the f8 shape (B = 1, Q = 900, T = 8, G = 4, P = 12, 6 cameras, 4 levels) against what gave the same
gradients before it: torch's autograd backward of the unfused route (the torch keypoint chain of plans.sampling_reference_ops'
kind + sampling_4d / rac_msmv_bwd_ex), and the forward kernel for scale.  _lib.timer events around the two kernels,
host-synchronised CUDA events around the autograd backward; batches of launches alternate between the candidates (DESIGN.md
section 3) so that clock and neighbours drift alike for all.  Writes one JSON record (default
profiles/sampling4d_core_bwd_f8.json; profiles/sampling4d_bwd_f8.json belongs to the sampling_4d operator).
    python tools/sampling4d_core_bwd_timing.py [--out PATH] [--rounds 6] [--batch 10]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import restate as R  # noqa: E402
from racformer_amd import _lib, synthetic as syn  # noqa: E402
from racformer_amd import transformer as T  # noqa: E402
from racformer_amd.bbox_utils import theta_d2xy_coods  # noqa: E402
from racformer_amd.fused import box_prep, sampling4d_backward, sampling4d_fused  # noqa: E402


def unfused(smp, qr, lin, feats, td, l2i, d_region, image_hw):
    """RaCFormerSampling.inner_forward (racformer_transformer.py:361-419) on the module's torch helpers and the
    differentiable sampling_4d"""
    B, Q, _ = qr.shape
    Tn, G, NP, D = smp.num_frames, smp.num_groups, smp.num_points, smp.depth_num
    off, ray, sc = lin
    pts = T.make_sample_points(theta_d2xy_coods(qr), off.reshape(B, Q, G * NP * D, 3), smp.pc_range).view(B, Q, 1, G, NP * D, 3)
    theta, dist = T._warp_to_polar(pts[..., 0:2], qr[..., 8:].detach(), td, smp.pc_range)
    base = torch.linspace(-d_region, d_region, D, device=qr.device)
    d_off = base + (torch.sigmoid(ray) * 2 - 1) * d_region / D / 2
    dist = (dist.view(B, Q, Tn, G, NP, D) + d_off[:, :, None, None, None, :]).reshape(B, Q, Tn, G, NP * D, 1)
    xy = theta_d2xy_coods(torch.cat([theta, dist], dim=-1))
    pc = smp.pc_range
    p3 = torch.cat([xy[..., 0:1] * (pc[3] - pc[0]) + pc[0], xy[..., 1:2] * (pc[4] - pc[1]) + pc[1],
                    pts[..., 2:3].expand(B, Q, Tn, G, NP * D, 1)], dim=-1)
    sw = torch.softmax(sc.view(B, Q, G, Tn, NP * D, smp.num_levels), dim=-1)
    return T.sampling_4d(p3, feats, sw, l2i, image_hw[0], image_hw[1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling4d_core_bwd_f8.json"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run cannot give a time"
    dev = "cuda:0"
    cfg = syn.F8
    tr = T.RaCFormerTransformer(**cfg.transformer_kwargs()).eval()
    syn.fill_params(tr, 22)
    tr = tr.to(dev)
    smp = tr.decoder.decoder_layer.sampling
    qb, qf = syn.make_queries(cfg, 21)
    qb, qf = qb.to(dev), (qf * 5.0).to(dev)
    metas = syn.make_img_metas(cfg)
    tr.decoder.stage_metas(metas, cfg.batch, torch.device(dev))
    td, l2i = metas[0]["time_diff"], metas[0]["lidar2img"]
    feats = [f.to(dev) for f in R.regroup_pyramid(syn.make_pyramid(cfg, 21), cfg.num_cams)]
    d_region = cfg.d_region_list[2]
    with torch.no_grad():
        lin = [x(qf) for x in (smp.sampling_offset, smp.ray_points_offset, smp.scale_weights)]
    table = box_prep(qb, smp.pc_range)
    args = (cfg.num_frames, cfg.num_groups, cfg.num_points, cfg.img_depth_num, smp.pc_range, d_region, cfg.image_hw[0], cfg.image_hw[1])
    P = cfg.num_points * cfg.img_depth_num
    gout = torch.randn(1, cfg.num_query, cfg.num_groups, cfg.num_frames * P, 64, device=dev)
    leaves = [x.clone().requires_grad_() for x in lin] + [qb.clone().requires_grad_()]
    gfeats = [f.clone().requires_grad_() for f in feats]
    names = ("sampling4d_bwd", "sampling4d_fwd")
    times = {"sampling4d_bwd": [], "sampling4d_fwd": [], "torch_autograd_bwd_of_unfused_route": [], "unfused_route_fwd": []}
    for r in range(a.rounds + 1):                     # round 0 warms every shape up and is dropped
        _lib.timer = _lib.KernelTimer(only=set(names))
        for _ in range(a.batch):
            sampling4d_backward(feats, qb, *lin, td, l2i, gout, *args, box_table=table)
        for _ in range(a.batch):
            sampling4d_fused(feats, qb, *lin, td, l2i, *args, box_table=table)
        torch.cuda.synchronize()
        kb, kf = (_lib.timer.mean_ms(n) for n in names)
        _lib.timer = None
        fw, bw = [], []
        for _ in range(a.batch):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            out = unfused(smp, leaves[3], leaves[:3], gfeats, td, l2i, d_region, cfg.image_hw)
            e[1].record()
            out.backward(gout)
            e[2].record()
            torch.cuda.synchronize()
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
            for x in leaves + gfeats:
                x.grad = None
        if r:
            times["sampling4d_bwd"].append(kb * 1e3)
            times["sampling4d_fwd"].append(kf * 1e3)
            times["torch_autograd_bwd_of_unfused_route"].append(float(np.median(bw)) * 1e3)
            times["unfused_route_fwd"].append(float(np.median(fw)) * 1e3)
    K = cfg.num_query * cfg.num_frames * cfg.num_groups * P
    rec = dict(shape=dict(B=1, Q=cfg.num_query, T=cfg.num_frames, G=cfg.num_groups, P=P, N=cfg.num_cams, L=cfg.num_levels, keypoints=K),
               method=f"{a.rounds} rounds of alternating batches of {a.batch} launches after one warm-up round; kernels: mean of HIP event "
                      "pairs around each launch (the zero-fill of grad_feats by the launcher lies outside them); torch autograd: median "
                      "of event pairs around backward() (its memsets, rac_msmv_bwd_ex and the elementwise chain); microseconds",
               us={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in times.items()},
               atomic_bytes_upper_bound=K * cfg.num_levels * 4 * 256,
               device=torch.cuda.get_device_name(0))
    rec["speedup_over_torch_autograd"] = rec["us"]["torch_autograd_bwd_of_unfused_route"]["median"] / rec["us"]["sampling4d_bwd"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec["us"], indent=1))
    print("speedup over torch autograd:", round(rec["speedup_over_torch_autograd"], 2))


if __name__ == "__main__":
    main()
