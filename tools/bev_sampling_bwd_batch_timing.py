#!/usr/bin/env python3
"""Time one BEV stream of the training route at the f8 shape with B = 2 (Q = 900, T = 8, 4 heads, P = 20, 128 x 128): forward +
backward of BEVSampling.attend_prepared through the fused route (fused_batch=True: rac_bev_sampling_fwd and
rac_bev_sampling_bwd_batch) and through forward_unfused (torch keypoint chain, rac_msda_fwd / rac_msda_bwd, torch frame fusion),
with the peak memory of each above what is live before the call, the two kernels on their own, and the B = 1 kernel
(rac_bev_sampling_bwd) for comparison with the commit before.  Host-synchronised CUDA events around forward + backward,
_lib.timer events around the kernels; batches alternate between the candidates.  Writes one JSON record
(default profiles/bev_sampling_bwd_batch_f8.json).
    python tools/bev_sampling_bwd_batch_timing.py [--out PATH] [--rounds 6] [--batch 10] [--parent-b1 JSON] [--errors JSON]
``--parent-b1``: the record tools/bev_sampling_bwd_timing.py wrote on the parent commit in the same session (its B = 1 kernel times
are copied in beside this commit's); ``--errors``: the worst err / A per gradient kind that tests/test_bev_sampling_batch_grad_gpu.py
wrote (RAC_BEV_BWD_BATCH_ERR_LOG)."""
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
from racformer_amd.fused import bev_sampling_backward, box_prep  # noqa: E402


def stats(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bev_sampling_bwd_batch_f8.json"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--parent-b1", default=None)
    ap.add_argument("--errors", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run cannot give a time"
    dev = "cuda:0"
    B, Q, heads, Tn, NP, D, H, W = 2, 900, 4, 8, 4, 5, 128, 128
    pc = list(syn.PC_RANGE)
    torch.manual_seed(3)
    m = T.BEVSampling(embed_dims=256, num_frames=Tn, num_points=NP, num_heads=heads, num_levels=1, pc_range=pc, spatial_shapes=(W, H),
                      depth_num=D).to(dev)
    with torch.no_grad():
        torch.nn.init.normal_(m.sampling_offset.weight, std=0.02)
    rng = np.random.default_rng(4)
    qr = rng.random((B, Q, 10), dtype=np.float32)
    qr[..., 1] = 0.05 + 0.55 * qr[..., 1]
    qr[..., 6:8] = qr[..., 6:8] * 2 - 1
    qr[..., 8:10] = qr[..., 8:10] * 4 - 2
    qr = torch.from_numpy(qr).to(dev).requires_grad_()
    qf = torch.randn(B, Q, 256, device=dev).requires_grad_()
    value = torch.randn(B * Tn, H * W, heads, 64, device=dev).requires_grad_()
    td = (torch.arange(Tn, device=dev, dtype=torch.float32) * 0.5)[None].repeat(B, 1).contiguous()
    gout = torch.randn(B, Q, 256, device=dev)
    table = box_prep(qr.detach(), pc)
    leaves = [qr, qf, value] + list(m.parameters())

    def route(fused):
        if fused:
            out = m.attend_prepared(qr, qf, value, (H, W), td, 0.1, box_table=table, fused_batch=True)
        else:
            out = m.forward_unfused(qr, qf, value, (H, W), td, 0.1)
        out.backward(gout)

    def timed_route(fused, n):
        ts = []
        for _ in range(n):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            route(fused)
            e[1].record()
            torch.cuda.synchronize()
            ts.append(e[0].elapsed_time(e[1]) * 1e3)
            for x in leaves:
                x.grad = None
        return float(np.median(ts))

    def peak(fused):
        for x in leaves:
            x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        route(fused)
        torch.cuda.synchronize()
        p = torch.cuda.max_memory_allocated() - base
        for x in leaves:
            x.grad = None
        return int(p)

    # the B = 1 kernel on the first sample's tensors (the shape and the draw of tools/bev_sampling_bwd_timing.py's measurement)
    with torch.no_grad():
        lin1 = [x(qf[:1]) for x in (m.sampling_offset, m.ray_points_offset, m.scale_weights, m.attention.bev_queue_weight)]
    v1, q1, t1, g1, tab1 = value.detach()[:Tn], qr.detach()[:1].contiguous(), td[:1].contiguous(), gout[:1].contiguous(), table[:1].contiguous()

    times = {"fused_route_fwd_bwd": [], "unfused_route_fwd_bwd": [], "bev_sampling_fwd_b2": [], "bev_sampling_bwd_batch_b2": [],
             "bev_sampling_bwd_b1": []}
    for r in range(a.rounds + 1):                     # round 0 warms every shape up and is dropped
        _lib.timer = _lib.KernelTimer(only={"bev_sampling_bwd", "bev_sampling_fwd"})
        tf = timed_route(True, a.batch)
        torch.cuda.synchronize()
        kb, kf = _lib.timer.mean_ms("bev_sampling_bwd"), _lib.timer.mean_ms("bev_sampling_fwd")
        _lib.timer = None
        tu = timed_route(False, a.batch)
        _lib.timer = _lib.KernelTimer(only={"bev_sampling_bwd"})
        for _ in range(2 * a.batch):
            bev_sampling_backward(v1, (H, W), q1, *lin1, t1, g1, Tn, heads, NP, D, pc, 0.1, box_table=tab1)
        torch.cuda.synchronize()
        k1 = _lib.timer.mean_ms("bev_sampling_bwd")
        _lib.timer = None
        if r:
            for k, v in (("fused_route_fwd_bwd", tf), ("unfused_route_fwd_bwd", tu), ("bev_sampling_fwd_b2", kf * 1e3),
                         ("bev_sampling_bwd_batch_b2", kb * 1e3), ("bev_sampling_bwd_b1", k1 * 1e3)):
                times[k].append(v)
    P = NP * D
    lds = 4 * B * (heads * Tn * P * 6 + heads * P * 8 + heads * 64 + Tn * 3 + 48)
    rec = dict(shape=dict(B=B, Q=Q, T=Tn, heads=heads, NP=NP, D=D, H=H, W=W, keypoints=B * Q * heads * Tn * P),
               method=f"{a.rounds} rounds of alternating batches after one warm-up round; routes: median of {a.batch} host-synchronised "
                      "event pairs around attend_prepared / forward_unfused + backward() of one stream (the four Linears, output_proj, "
                      "the memset of grad_value included); kernels: mean of HIP event pairs around each launch; microseconds; peak "
                      "memory: torch.cuda.max_memory_allocated over one forward + backward above what was allocated before it",
               us={k: stats(v) for k, v in times.items()},
               peak_bytes=dict(fused_route=peak(True), unfused_route=peak(False)),
               lds_bytes_per_workgroup=lds, workgroups_per_cu_by_lds=160 * 1024 // lds,
               atomic_bytes=B * Q * heads * Tn * P * 4 * 256,
               device=torch.cuda.get_device_name(0))
    rec["fused_over_unfused"] = rec["us"]["unfused_route_fwd_bwd"]["median"] / rec["us"]["fused_route_fwd_bwd"]["median"]
    if a.parent_b1:
        with open(a.parent_b1) as f:
            parent = json.load(f)
        rec["bev_sampling_bwd_b1_parent_commit"] = dict(note="tools/bev_sampling_bwd_timing.py of the parent commit, same session",
                                                        us=parent["us"]["bev_sampling_bwd"], bev_sampling_fwd_us=parent["us"]["bev_sampling_fwd"])
    if a.errors:
        with open(a.errors) as f:
            rec["error_vs_float64"] = dict(note="worst |got - ref| / A over tests/test_bev_sampling_batch_grad_gpu.py::"
                                                "test_kernel_against_float64, in units of 2**-24; A = the same sums with every term "
                                                "non-negative", **json.load(f))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps({k: rec[k] for k in ("us", "peak_bytes", "fused_over_unfused")}, indent=1))


if __name__ == "__main__":
    main()
