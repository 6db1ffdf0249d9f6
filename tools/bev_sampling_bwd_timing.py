#!/usr/bin/env python3
"""Time rac_bev_sampling_bwd at the f8 shape (B = 1, Q = 900, T = 8, 4 heads, P = 20, 128 x 128) against what gave the same
gradients before it: torch's autograd backward of BEVSampling.forward_unfused (torch keypoint chain + rac_msda_bwd + frame
fusion), and the forward kernel for scale.  _lib.timer events around the two kernels, host-synchronised CUDA events around the
autograd backward; batches of launches alternate between the candidates so that clock and neighbours
drift alike for all.  Writes one JSON record (default profiles/bev_sampling_bwd_f8.json).
    python tools/bev_sampling_bwd_timing.py [--out PATH] [--rounds 6] [--batch 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from racformer_amd import _lib, synthetic as syn  # noqa: E402
from racformer_amd import transformer as T  # noqa: E402
from racformer_amd.fused import bev_sampling_backward, bev_sampling_fused, box_prep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bev_sampling_bwd_f8.json"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run cannot give a time"
    dev = "cuda:0"
    Q, heads, Tn, NP, D, H, W = 900, 4, 8, 4, 5, 128, 128
    pc = list(syn.PC_RANGE)
    torch.manual_seed(3)
    m = T.BEVSampling(embed_dims=256, num_frames=Tn, num_points=NP, num_heads=heads, num_levels=1, pc_range=pc, spatial_shapes=(W, H),
                      depth_num=D).to(dev)
    with torch.no_grad():
        torch.nn.init.normal_(m.sampling_offset.weight, std=0.02)
    rng = np.random.default_rng(4)
    qr = rng.random((1, Q, 10), dtype=np.float32)
    qr[..., 1] = 0.05 + 0.55 * qr[..., 1]
    qr[..., 6:8] = qr[..., 6:8] * 2 - 1
    qr[..., 8:10] = qr[..., 8:10] * 4 - 2
    qr = torch.from_numpy(qr).to(dev)
    qf = torch.randn(1, Q, 256, device=dev)
    value = torch.randn(Tn, H * W, heads, 64, device=dev)
    td = (torch.arange(Tn, device=dev, dtype=torch.float32) * 0.5)[None]
    gout = torch.randn(1, Q, 256, device=dev)
    with torch.no_grad():
        lin = [x(qf) for x in (m.sampling_offset, m.ray_points_offset, m.scale_weights, m.attention.bev_queue_weight)]
    table = box_prep(qr, pc)
    cfg = (Tn, heads, NP, D, pc, 0.1)

    def fused_bwd():
        bev_sampling_backward(value, (H, W), qr, *lin, td, gout, *cfg, box_table=table)

    def fused_fwd():
        bev_sampling_fused(value, (H, W), qr, *lin, td, *cfg, box_table=table)

    # (b): leaves = the value stream, the four Linear outputs and the boxes; backward of the unfused core only (no output_proj)
    leaves = [value.clone().requires_grad_()] + [x.clone().requires_grad_() for x in lin[:3]] + [qr.clone().requires_grad_()]
    qfl = qf.clone().requires_grad_()

    def unfused_graph():
        loc, sw = m.keypoints(leaves[4], qfl, td, 0.1, (leaves[1], leaves[2], leaves[3]))
        return m.attention.attend(qfl, leaves[0], loc, sw, (H, W))

    times = {"bev_sampling_bwd": [], "bev_sampling_fwd": [], "torch_autograd_bwd_of_forward_unfused": [], "forward_unfused_fwd": []}
    for r in range(a.rounds + 1):                     # round 0 warms every shape up and is dropped
        _lib.timer = _lib.KernelTimer(only={"bev_sampling_bwd", "bev_sampling_fwd"})
        for _ in range(a.batch):
            fused_bwd()
        for _ in range(a.batch):
            fused_fwd()
        torch.cuda.synchronize()
        kb, kf = _lib.timer.mean_ms("bev_sampling_bwd"), _lib.timer.mean_ms("bev_sampling_fwd")
        _lib.timer = None
        fw, bw = [], []
        for _ in range(a.batch):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            out = unfused_graph()
            e[1].record()
            out.backward(gout)
            e[2].record()
            torch.cuda.synchronize()
            fw.append(e[0].elapsed_time(e[1]))
            bw.append(e[1].elapsed_time(e[2]))
            for x in leaves + [qfl] + list(m.parameters()):
                x.grad = None
        if r:
            times["bev_sampling_bwd"].append(kb * 1e3)
            times["bev_sampling_fwd"].append(kf * 1e3)
            times["torch_autograd_bwd_of_forward_unfused"].append(float(np.median(bw)) * 1e3)
            times["forward_unfused_fwd"].append(float(np.median(fw)) * 1e3)
    rec = dict(shape=dict(B=1, Q=Q, T=Tn, heads=heads, NP=NP, D=D, H=H, W=W, keypoints=Q * heads * Tn * NP * D),
               method=f"{a.rounds} rounds of alternating batches of {a.batch} launches after one warm-up round; kernels: mean of HIP event "
                      "pairs around each launch; torch autograd: median of event pairs around backward() (its memset of grad_value, "
                      "rac_msda_bwd and the elementwise chain; includes output_proj's and the frame Linear's backward); microseconds",
               us={k: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v))) for k, v in times.items()},
               atomic_bytes=Q * heads * Tn * NP * D * 4 * 256,
               device=torch.cuda.get_device_name(0))
    rec["speedup_over_torch_autograd"] = rec["us"]["torch_autograd_bwd_of_forward_unfused"]["median"] / rec["us"]["bev_sampling_bwd"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec["us"], indent=1))
    print("speedup over torch autograd:", round(rec["speedup_over_torch_autograd"], 2))


if __name__ == "__main__":
    main()
