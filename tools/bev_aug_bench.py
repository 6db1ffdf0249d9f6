#!/usr/bin/env python3
"""Timing of the BEV augmentation (racformer_amd/bev_aug.py) on the f8 shapes: per sample 8 radar clouds of about 1 500 points x 7,
one lidar cloud of about 34 000 points x 5 and 30 boxes x 9, for B = 1 and B = 2 samples.  Needs the GPU.

    python tools/bev_aug_bench.py [--out profiles/bev_aug_f8.json]

Two ways to the same rows on the same inputs, after a warm-up; times in microseconds, median with the 10th and 90th percentile:
  hip    launch_eager / launch_graph: ``rac_bev_aug_fwd`` alone on a plan and buffers that stay put (device events);
         prepare_bev_aug: the whole ``RaCFormer.prepare_bev_aug`` call on device tensors -- the draws, the 48 view matrices, the tables
         and their upload, the launch -- as device events around the call and as wall clock with a synchronisation at its end
  host   what the route replaces: ``bev_aug_torch`` on CPU tensors for every cloud and box set (wall clock, 16 threads) and the upload
         of the results from pinned memory (device events)
The method uses nothing of the detector, so it is called unbound here: no weights are built."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from racformer_amd import bev_aug as A, synthetic as syn  # noqa: E402
from racformer_amd.detector import RaCFormer  # noqa: E402

T, VIEWS, HW = 8, 6, (256, 704)
N_RADAR, N_LIDAR, N_BOXES = 1500, 34000, 30


def spread(v):
    v = sorted(v)
    return dict(median=round(statistics.median(v), 2), p10=round(v[len(v) // 10], 2), p90=round(v[(9 * len(v)) // 10], 2))


def timed(fns, reps, warmup=5):
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
    return {k: spread([1e3 * a.elapsed_time(b) for a, b in v]) for k, v in ev.items()}


def wall(f, reps, warmup=2, sync=False):
    out = []
    for i in range(warmup + reps):
        t0 = time.perf_counter()
        f()
        if sync:
            torch.cuda.synchronize()
        if i >= warmup:
            out.append(1e6 * (time.perf_counter() - t0))
    return spread(out)


def sample(seed):
    """One sample's clouds and boxes: points around the ego vehicle 1 to 80 m out, boxes inside the recipe's range."""
    rng = np.random.default_rng(seed)

    def cloud(n, width):
        r, phi = rng.uniform(1.0, 80.0, n), rng.uniform(-np.pi, np.pi, n)
        xyz = np.stack([r * np.cos(phi), r * np.sin(phi), rng.uniform(-2.0, 2.0, n)], axis=1)
        return torch.from_numpy(np.concatenate([xyz, rng.normal(0, 8, (n, width - 3))], axis=1).astype(np.float32))

    radar = [cloud(N_RADAR + int(rng.integers(-100, 100)), 7) for _ in range(T)]
    boxes = torch.from_numpy(np.concatenate([rng.uniform(-50, 50, (N_BOXES, 2)), rng.uniform(-2, 0, (N_BOXES, 1)), rng.uniform(0.5, 5, (N_BOXES, 3)),
                                             rng.uniform(-3.14, 3.14, (N_BOXES, 1)), rng.normal(0, 3, (N_BOXES, 2))], axis=1).astype(np.float32))
    return radar, cloud(N_LIDAR + int(rng.integers(-500, 500)), 5), boxes


def bench(B, dev, reps, host_reps):
    samples = [sample(10 + b) for b in range(B)]
    radar = [[samples[b][0][t] for b in range(B)] for t in range(T)]
    lidar, boxes = [s[1] for s in samples], [s[2] for s in samples]
    metas = [dict(lidar2img=[np.asarray(m, np.float64) for m in np.asarray(syn.ring_lidar2img(T, VIEWS, image_hw=HW)).reshape(-1, 4, 4)])
             for _ in range(B)]
    transform = A.RaCGlobalRotScaleTransImage()
    np.random.seed(1)
    draws = [transform.draw() for _ in range(B)]
    on = lambda xs: [x.to(dev) for x in xs]                                 # noqa: E731
    radar_d, lidar_d, boxes_d = [on(f) for f in radar], on(lidar), on(boxes)

    # the launch alone: a plan on buffers that stay put
    groups = [([radar_d[t][b] for b in range(B) for t in range(T)], [b for b in range(B) for _ in range(T)], "points"),
              (lidar_d, list(range(B)), "points"), (boxes_d, list(range(B)), "boxes")]
    segments, outs = [], []
    for srcs, smp, kind in groups:
        packed = torch.empty(sum(s.shape[0] for s in srcs), srcs[0].shape[1], device=dev)
        at = 0
        for s, b in zip(srcs, smp):
            segments.append((s, packed[at:at + s.shape[0]], kind, b))
            outs.append((packed[at:at + s.shape[0]], s, kind, b))
            at += s.shape[0]
    plan = A.BevAugPlan(segments, B)
    table = A.draw_table(draws, dev)
    plan.launch(table)
    torch.cuda.synchronize()
    equal = all(torch.equal(o.cpu().view(torch.int32), A.bev_aug_torch(s.cpu(), A.draw_row(draws[b]), kind).view(torch.int32))
                for o, s, kind, b in outs)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        plan.launch(table)

    def prepare():
        return RaCFormer.prepare_bev_aug(None, metas, radar_d, lidar_d, boxes_d, transform=transform, draws=draws)

    times = timed({"launch_eager": lambda: plan.launch(table), "launch_graph": graph.replay, "prepare_bev_aug": prepare}, reps)
    times["prepare_bev_aug_wall"] = wall(prepare, reps, sync=True)
    times["view_mats_wall"] = wall(lambda: [A.view_mats(m["lidar2img"], d) for m, d in zip(metas, draws)], host_reps)

    # what the route replaces: the rule on the host, then the uploads from pinned memory
    host_groups = [([radar[t][b] for b in range(B) for t in range(T)], groups[0][1], "points"), (lidar, groups[1][1], "points"),
                   (boxes, groups[2][1], "boxes")]

    def host_rule():
        return [A.bev_aug_torch(s, A.draw_row(draws[b]), kind) for srcs, smp, kind in host_groups for s, b in zip(srcs, smp)]

    times["host_rule_cpu"] = wall(host_rule, host_reps)
    pinned = [t.pin_memory() for t in host_rule()]
    targets = [torch.empty_like(t, device=dev) for t in pinned]
    times.update(timed({"host_uploads": lambda: [d.copy_(p, non_blocking=True) for d, p in zip(targets, pinned)]}, reps))
    rows = dict(radar=sum(s.shape[0] for s in groups[0][0]), lidar=sum(s.shape[0] for s in lidar), boxes=sum(s.shape[0] for s in boxes))
    nbytes = 2 * 4 * (rows["radar"] * 7 + rows["lidar"] * 5 + rows["boxes"] * 9)
    return dict(B=B, rows=rows, segments=plan.n_segs, chunks=plan.n_chunks, bytes_read_and_written=nbytes, times=times,
                hip_equals_cpu_restatement_bitwise=bool(equal))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "bev_aug_f8.json"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bev_aug_bench needs the MI355X"
    torch.set_num_threads(args.threads)
    rec = dict(shape=dict(frames=T, views=VIEWS, radar_points=N_RADAR, lidar_points=N_LIDAR, boxes=N_BOXES),
               device=torch.cuda.get_device_name(0), host_threads=torch.get_num_threads(), reps=args.reps, host_reps=args.host_reps,
               unit="us; device-event times (*_wall and host_rule_cpu: wall clock), median / p10 / p90, routes alternating inside every repetition",
               runs=[bench(B, "cuda:0", args.reps, args.host_reps) for B in (1, 2)])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
