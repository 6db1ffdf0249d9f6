#!/usr/bin/env python3
"""Timing of the LSS depth branch (racformer_amd/lss_depth.py) on the f8 shape: B = 1, 6 cameras, 256 x 704 maps, ds = 16
(4224 feature pixels), D = 96, 64 RCS classes, 32 embedding channels.  Needs the GPU.

    python tools/lss_depth_bench.py [--out profiles/lss_depth_f8.json] [--errors lss_depth_errors.json]

One step = pooling of the radar depth and RCS maps + the prior tensor + the embedding's gradients + pooling of the lidar depth map
+ the depth loss + its gradient.  Two routes on the same device and the same inputs, alternating inside every repetition, after a
warm-up, medians of device-event times in microseconds:
  hip     the kernels (rac_lss_*), eager and as a captured graph; every entry point also alone
  torch   the torch restatement of racformer_amd/lss_depth.py under autograd (the reference's operations: pooling through
          view / permute / min, boolean-mask gather and Python max() on a device tensor -- two host syncs, so it cannot be
          captured), eager only
Launch counts: the kernels are counted from the route itself; torch's from torch.profiler's device-kernel events of one step.
--errors: the (E_ref, kernel error) pairs a `RAC_LSS_DEPTH_ERRORS=<file> pytest -m gpu tests/test_lss_depth_gpu.py` session
wrote, copied into the record.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from racformer_amd import lss_depth as LD, synthetic as syn  # noqa: E402

GRID = dict(depth=[1.0, 65.0, 96.0], rcs=[-64, 64, 64])
DS, D, E, N_RCS = 16, 96, 32, 64
ALPHA, GAMMA, WEIGHT = 0.25, 2.0, 2.0
HIP_LAUNCHES = dict(rac_lss_pool_bins_fwd=2, rac_lss_prior_fwd=1, rac_lss_prior_bwd=2, rac_lss_depth_loss_fwd=2, rac_lss_depth_loss_bwd=1)


def timed(fns, reps, warmup=10):
    """{name: median us}; the functions alternate inside every repetition"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: round(1e3 * statistics.median(a.elapsed_time(b) for a, b in v), 2) for k, v in ev.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "lss_depth_f8.json"))
    ap.add_argument("--errors", default=None)
    ap.add_argument("--reps", type=int, default=300)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lss_depth_bench needs the MI355X"
    dev = "cuda:0"
    inp = syn.make_lss_depth_inputs(seed=3)
    radar_depth, radar_rcs, lidar = (inp[k].to(dev) for k in ("radar_depth", "radar_rcs", "lidar_depth"))
    bn, H, W = radar_depth.shape
    h, w = H // DS, W // DS
    logits = torch.from_numpy(syn.rng_normal(5, (bn, D, h, w), scale=2.0)).to(dev)
    weight = torch.from_numpy(syn.rng_normal(6, (E, N_RCS, 1, 1))).to(dev)
    bias = torch.from_numpy(syn.rng_normal(7, (E,))).to(dev)
    gout = torch.from_numpy(syn.rng_normal(8, (bn, D + 1 + E, h, w))).to(dev)
    one = torch.ones(1, device=dev)

    def hip_step():
        _, bins, cls = LD.pool_bins(radar_depth, radar_rcs, GRID, DS)
        prior = LD.radar_prior_forward(bins, cls, weight, bias, D)
        gw, gb = LD.radar_prior_backward(gout, cls, D, E, N_RCS)
        _, labels, _ = LD.pool_bins(lidar, None, GRID, DS)
        loss, unit, scale = LD.depth_loss_forward(logits, labels, ALPHA, GAMMA, WEIGHT)
        return prior, gw, gb, loss, LD.depth_loss_backward(one, unit, scale)

    def torch_step():
        wt, bs, lg = weight.requires_grad_(True), bias.requires_grad_(True), logits.requires_grad_(True)
        _, bins, cls = LD.pool_bins_torch(radar_depth, radar_rcs, GRID, DS)
        prior = LD.radar_prior_torch(bins, cls, wt, bs, D)
        gw, gb = torch.autograd.grad(prior, (wt, bs), gout)
        _, labels, _ = LD.pool_bins_torch(lidar, None, GRID, DS)
        loss = LD.depth_loss_torch(lg, labels, ALPHA, GAMMA, WEIGHT)
        (grad,) = torch.autograd.grad(loss, lg)
        return prior.detach(), gw, gb, loss.detach(), grad

    ours, theirs = hip_step(), torch_step()
    torch.cuda.synchronize()
    agree = {k: float((a.reshape(-1) - b.reshape(-1)).abs().max()) for k, a, b in zip(("prior", "grad_weight", "grad_bias", "loss", "grad_logits"),
                                                                                      ours, theirs)}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(3):
            hip_step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        captured = hip_step()
    graph.replay()
    torch.cuda.synchronize()
    graph_equals_eager = all(torch.equal(a, b) for a, b in zip(captured, ours))

    times = timed({"hip_eager": hip_step, "hip_graph": graph.replay, "torch_eager": torch_step}, args.reps)
    # ---- every entry point alone (eager, allocations included)
    _, bins, cls = LD.pool_bins(radar_depth, radar_rcs, GRID, DS)
    _, labels, _ = LD.pool_bins(lidar, None, GRID, DS)
    _, unit, scale = LD.depth_loss_forward(logits, labels, ALPHA, GAMMA, WEIGHT)
    entry_points = timed({
        "rac_lss_pool_bins_fwd(depth, rcs)": lambda: LD.pool_bins(radar_depth, radar_rcs, GRID, DS),
        "rac_lss_pool_bins_fwd(depth)": lambda: LD.pool_bins(lidar, None, GRID, DS),
        "rac_lss_prior_fwd": lambda: LD.radar_prior_forward(bins, cls, weight, bias, D),
        "rac_lss_prior_bwd": lambda: LD.radar_prior_backward(gout, cls, D, E, N_RCS),
        "rac_lss_depth_loss_fwd": lambda: LD.depth_loss_forward(logits, labels, ALPHA, GAMMA, WEIGHT),
        "rac_lss_depth_loss_bwd": lambda: LD.depth_loss_backward(one, unit, scale),
    }, args.reps)
    rec = dict(shape=dict(maps=bn, H=H, W=W, ds=DS, pixels=bn * h * w, D=D, rcs_classes=N_RCS, embedding=E,
                          foreground=int((LD.pool_bins(lidar, None, GRID, DS)[1] < D).sum())),
               device=torch.cuda.get_device_name(0), unit="us, median of device-event times around one step", reps=args.reps,
               step="pool(radar depth, rcs) + prior fwd + prior bwd + pool(lidar depth) + depth loss fwd + bwd",
               times=times, entry_points=entry_points, launches=dict(hip=sum(HIP_LAUNCHES.values()), hip_by_entry_point=HIP_LAUNCHES, torch_device_kernels="not measured"),
               hip_vs_torch_max_abs_diff=agree, graph_replay_equals_eager_bitwise=graph_equals_eager)
    if args.errors and os.path.exists(args.errors):
        rec["tolerance_bases"] = json.load(open(args.errors))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def write():
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)

    write()                                                   # (the timings are on disk before the profiler is started)
    try:
        acts = [torch.profiler.ProfilerActivity.CPU, torch.profiler.ProfilerActivity.CUDA]
        with torch.profiler.profile(activities=acts) as prof:
            torch_step()
            torch.cuda.synchronize()
        rec["launches"]["torch_device_kernels"] = sum(e.count for e in prof.key_averages()
                                                      if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as exc:                                  # a rig without a working tracer: the count stays unmeasured
        rec["launches"]["torch_device_kernels"] = f"not measured ({type(exc).__name__})"
    write()
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
