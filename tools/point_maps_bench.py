#!/usr/bin/env python3
"""Timing of the point maps (racformer_amd/point_maps.py) on the f8 shape: 8 radar clouds of about 1 500 points x 6 views -> 48
radar_depth and 48 radar_rcs maps of 256 x 704, and one lidar cloud of about 34 000 points x 6 views -> 6 gt_depth maps.  Needs the GPU.

    python tools/point_maps_bench.py [--out profiles/point_maps_f8.json]

Three ways to the same maps on the same inputs, alternating inside every repetition after a warm-up; device-event times in
microseconds, median with the 10th and 90th percentile:
  hip        rac_point_maps_radar_fwd / rac_point_maps_lidar_fwd on buffers that stay put, eager and as a captured graph
  torch_dev  the torch restatement on the device (eager: it reads the kept count back per view, so it cannot be captured)
  host       what the route replaces: the restatement on the CPU (wall clock, the threads torch is given) and the upload of the
             maps -- [48, 256, 704] x 2 float32 for the radar, [6, 256, 704] for the lidar -- from pinned memory (device events)
Also recorded: the streaming step's share, 6 maps of one 1 500-point cloud (the one-frame front end of the detector)."""
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

from racformer_amd import point_maps as PM, synthetic as syn  # noqa: E402

GRID = dict(depth=[1.0, 65.0, 96.0])
HW, VIEWS = (256, 704), 6


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


def clouds(n_clouds, n_points, seed, width):
    """Points in front of and around a six-camera ring, 1 to 80 m out (some beyond the depth range, most views see a sixth of them)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_clouds):
        r, phi = rng.uniform(1.0, 80.0, n_points), rng.uniform(-np.pi, np.pi, n_points)
        xyz = np.stack([r * np.cos(phi), r * np.sin(phi), rng.uniform(-2.0, 2.0, n_points)], axis=1)
        out.append(torch.from_numpy(np.concatenate([xyz, rng.normal(0, 8, (n_points, width - 3))], axis=1).astype(np.float32)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "point_maps_f8.json"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "point_maps_bench needs the MI355X"
    dev = "cuda:0"
    T = 8
    l2i = syn.ring_lidar2img(T, VIEWS, image_hw=HW)
    mats = PM.view_table(np.asarray(l2i).reshape(-1, 4, 4))
    rp, ro = PM.pack_clouds(clouds(T, 1500, 1, 7))
    lp, lo = PM.pack_clouds(clouds(1, 34000, 2, 5))
    rpd, rod, rmd, lpd, lod, lmd = rp.to(dev), ro.to(dev), mats.to(dev), lp.to(dev), lo.to(dev), mats[:VIEWS].to(dev)
    one_p, one_o = PM.pack_clouds([rp[:1500]])
    one_pd, one_od = one_p.to(dev), one_o.to(dev)

    depth, rcs = (torch.empty(T * VIEWS, *HW, device=dev) for _ in range(2))
    gt = torch.empty(VIEWS, *HW, device=dev)
    rs = torch.empty(PM.radar_scratch_words(T * VIEWS, HW[1]), dtype=torch.int64, device=dev)
    ls = torch.empty(PM.lidar_scratch_words(VIEWS, *HW), dtype=torch.int64, device=dev)
    d1, r1 = depth[:VIEWS], rcs[:VIEWS]

    def hip_radar():
        PM.radar_maps_fwd(rpd, rod, rmd, HW, 1.0, 65.0, depth=depth, rcs=rcs, scratch=rs)

    def hip_lidar():
        PM.lidar_depth_map_fwd(lpd, lod, lmd, HW, 1.0, 65.0, out=gt, scratch=ls)

    def hip_one_frame():
        PM.radar_maps_fwd(one_pd, one_od, lmd, HW, 1.0, 65.0, depth=d1, rcs=r1, scratch=rs)

    hip_radar(), hip_lidar()
    torch.cuda.synchronize()
    want_r = PM.radar_maps_torch(rp, ro, mats, HW, GRID)
    want_l = PM.lidar_depth_map_torch(lp, lo, mats[:VIEWS], HW, GRID)
    equal = dict(radar_depth=torch.equal(depth.cpu(), want_r[0]), radar_rcs=torch.equal(rcs.cpu(), want_r[1]), gt_depth=torch.equal(gt.cpu(), want_l))
    occupied = dict(radar_columns=int((want_r[0][:, 0] != 0).sum()), lidar_pixels=int((want_l != 0).sum()))

    graphs = {}
    for name, fn in (("radar", hip_radar), ("lidar", hip_lidar), ("one_frame", hip_one_frame)):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        graphs[name] = g
    times = timed({
        "hip_radar_eager": hip_radar, "hip_radar_graph": graphs["radar"].replay,
        "hip_lidar_eager": hip_lidar, "hip_lidar_graph": graphs["lidar"].replay,
        "hip_one_frame_eager": hip_one_frame, "hip_one_frame_graph": graphs["one_frame"].replay,
    }, args.reps)
    times.update(timed({
        "torch_dev_radar": lambda: PM.radar_maps_torch(rpd, rod, rmd, HW, GRID),
        "torch_dev_lidar": lambda: PM.lidar_depth_map_torch(lpd, lod, lmd, HW, GRID),
    }, max(args.reps // 10, 3), warmup=2))

    # what the route replaces: the maps made on the host, then uploaded from pinned memory
    pin_r = [torch.empty(T * VIEWS, *HW).pin_memory() for _ in range(2)]
    pin_l = torch.empty(VIEWS, *HW).pin_memory()
    host = {k: [] for k in ("host_radar_cpu", "host_lidar_cpu", "host_one_frame_cpu")}
    for _ in range(args.host_reps):
        for k, f in (("host_radar_cpu", lambda: PM.radar_maps_torch(rp, ro, mats, HW, GRID)),
                     ("host_lidar_cpu", lambda: PM.lidar_depth_map_torch(lp, lo, mats[:VIEWS], HW, GRID)),
                     ("host_one_frame_cpu", lambda: PM.radar_maps_torch(one_p, one_o, mats[:VIEWS], HW, GRID))):
            t0 = time.perf_counter()
            f()
            host[k].append(1e6 * (time.perf_counter() - t0))
    times.update({k: spread(v) for k, v in host.items()})
    times.update(timed({
        "upload_radar_2x48_maps": lambda: (depth.copy_(pin_r[0], non_blocking=True), rcs.copy_(pin_r[1], non_blocking=True)),
        "upload_lidar_6_maps": lambda: gt.copy_(pin_l, non_blocking=True),
        "upload_one_frame_2x6_maps": lambda: (d1.copy_(pin_r[0][:VIEWS], non_blocking=True), r1.copy_(pin_r[1][:VIEWS], non_blocking=True)),
    }, args.reps))

    rec = dict(shape=dict(radar=dict(clouds=T, points=int(rp.shape[0]), views=VIEWS, maps=T * VIEWS, hw=HW),
                          lidar=dict(points=int(lp.shape[0]), views=VIEWS, hw=HW), one_frame=dict(points=1500, views=VIEWS)),
               device=torch.cuda.get_device_name(0), host_threads=torch.get_num_threads(), reps=args.reps, host_reps=args.host_reps,
               unit="us; device-event times (host_*_cpu: wall clock), median / p10 / p90, routes alternating inside every repetition",
               times=times, hip_equals_cpu_restatement_bitwise=equal, occupied=occupied,
               bytes=dict(radar_maps=2 * T * VIEWS * HW[0] * HW[1] * 4, lidar_maps=VIEWS * HW[0] * HW[1] * 4))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
