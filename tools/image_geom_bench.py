#!/usr/bin/env python3
"""Timing of the geometric image augmentation (racformer_amd/image_geom.py) on the f8 shape: the 48 raw frames of one sample,
900 x 1600 x 3 uint8 and resident on the device, to 48 images of 256 x 704 -- at the two ends of the recipe's resize_lim (0.38: the
strongest down-scale, the image narrower than the window; 0.55: flipped, cropped on every side) and at the test-mode record (0.44).
Needs the GPU.

    python tools/image_geom_bench.py [--out profiles/image_geom_f8.json]

Per record and output kind (microseconds, median / p10 / p90):
  launch   rac_image_geom_fwd alone on tables and an output that stay put, eager and as a captured graph's replay: device events,
           alternating inside every repetition after a warm-up
  call     ``transform_images`` as a user calls it -- the tables made and uploaded, the output allocated, the launch -- on the host
           clock from the call to the end of a synchronise
and, on the same host clock: the tables' construction (``geometry_tables``) and their upload, each by itself.
``bytes``: what the algorithm has to move -- the raw rows and columns some output position reads, once, plus the output -- and the
time those bytes take at 8 TB/s over the launch's time.  ``host``: what the route replaces, the 48 frames through Pillow (where it
is installed; else through the numpy restatement) on 16 threads, wall clock."""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from racformer_amd import image_geom as G  # noqa: E402

RAW_HW, FINAL, N_IMAGES, HOST_THREADS, HBM_BYTES_PER_S = (900, 1600), (256, 704), 48, 16, 8.0e12
F8_CONF = dict(H=900, W=1600, final_dim=FINAL, resize_lim=(0.38, 0.55), bot_pct_lim=(0.0, 0.0), rot_lim=(0.0, 0.0), rand_flip=True)


def records():
    def at(resize, flip):
        new_w, new_h = int(RAW_HW[1] * resize), int(RAW_HW[0] * resize)
        crop_w, crop_h = max(0, new_w - FINAL[1]) // 2, new_h - FINAL[0]
        return G.IdaDraw(resize, (new_w, new_h), (crop_w, crop_h, crop_w + FINAL[1], crop_h + FINAL[0]), flip, 0.0)

    return {"resize_0.38": at(0.38, False), "resize_0.55_flipped": at(0.55, True),
            "test_mode_0.44": G.RandomTransformImage(F8_CONF, training=False).draw()}


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


def host_clock(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e6 * (time.perf_counter() - t0))
    return spread(out)


def algorithmic_bytes(draw):
    """Raw bytes some output position reads (rows x columns x 3, per image, counted once) and the output's bytes per kind."""
    tab, _ = G.geometry_tables([draw], RAW_HW)
    fH, fW = FINAL
    hb, vb = tab[0, :2 * fW].reshape(fW, 2), tab[0, 2 * fW:2 * (fW + fH)].reshape(fH, 2)

    def touched(bounds, size):
        seen = np.zeros(size, bool)
        for lo, cnt in bounds:
            seen[lo:lo + cnt] = True
        return int(seen.sum())

    rows, cols = touched(vb, RAW_HW[0]), touched(hb, RAW_HW[1])
    return dict(raw_rows=rows, raw_columns=cols, raw=N_IMAGES * rows * cols * 3, out_f32_chw=N_IMAGES * 3 * fH * fW * 4, out_u8_hwc=N_IMAGES * 3 * fH * fW)


def host_route(raw_np, draw, reps):
    try:
        from PIL import Image

        def one(im):
            im = Image.fromarray(im).resize(draw.resize_dims).crop(draw.crop)
            if draw.flip:
                im = im.transpose(method=Image.FLIP_LEFT_RIGHT)
            return np.array(im.rotate(draw.rotate))
        name = "Pillow " + __import__("PIL").__version__
    except ImportError:
        one, name = (lambda im: G.transform_images_numpy(im[None], draw)[0]), "numpy restatement"
    times = []
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        for _ in range(reps):
            t0 = time.perf_counter()
            res = list(pool.map(one, raw_np))
            times.append(1e6 * (time.perf_counter() - t0))
    return name, spread(times), np.stack(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "image_geom_f8.json"))
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "image_geom_bench needs the MI355X"
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    raw_np = rng.integers(0, 256, (N_IMAGES,) + RAW_HW + (3,), dtype=np.uint8)
    raw = torch.from_numpy(raw_np).to(dev)
    outs = {"f32_chw": torch.empty(N_IMAGES, 3, *FINAL, device=dev), "u8_hwc": torch.empty(N_IMAGES, *FINAL, 3, dtype=torch.uint8, device=dev)}
    rec = dict(shape=dict(images=N_IMAGES, raw_hw=RAW_HW, final_hw=FINAL), device=torch.cuda.get_device_name(0), reps=args.reps,
               host_reps=args.host_reps, host_threads=HOST_THREADS,
               unit="us; launch_*: device-event times, routes alternating inside every repetition; call_*, tables_*, host_*: wall clock "
                    "to the end of a synchronise; median / p10 / p90", records={})
    for name, draw in records().items():
        tables = G.device_tables([draw], RAW_HW, dev)
        fns, graphs = {}, []
        for kind, out in outs.items():
            launch = lambda kind=kind, out=out: G.image_geom_fwd(raw, [draw], kind, into=out, tables=tables)       # noqa: E731
            launch()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                launch()
            graphs.append(g)
            fns[f"launch_{kind}_eager"], fns[f"launch_{kind}_graph"] = launch, g.replay
        times = timed(fns, args.reps)
        for kind in outs:           # (host work in front of the launch: the host clock, not device events)
            times[f"call_{kind}"] = host_clock(lambda kind=kind: G.transform_images(raw, [draw], out=kind), 20)
        times["tables_construction_host"] = host_clock(lambda: G.geometry_tables([draw], RAW_HW), 20)
        times["tables_upload"] = host_clock(lambda: torch.from_numpy(tables.host).to(dev), 20)
        host_name, host_time, host_out = host_route(raw_np, draw, args.host_reps)
        times["host_48_frames"] = host_time
        G.image_geom_fwd(raw, [draw], "u8_hwc", into=outs["u8_hwc"], tables=tables)
        G.image_geom_fwd(raw, [draw], "f32_chw", into=outs["f32_chw"], tables=tables)
        u8 = outs["u8_hwc"].cpu().numpy()
        equal = dict(u8_equals_host_route=bool(np.array_equal(u8, host_out)),
                     f32_equals_u8=bool(np.array_equal(outs["f32_chw"].cpu().numpy(), u8.transpose(0, 3, 1, 2).astype(np.float32))),
                     first_frame_equals_numpy_restatement=bool(np.array_equal(u8[:1], G.transform_images_numpy(raw_np[:1], draw))))
        nbytes = algorithmic_bytes(draw)
        roof = {}
        for kind in outs:
            total = nbytes["raw"] + nbytes[f"out_{kind}"]
            t = times[f"launch_{kind}_graph"]["median"]
            roof[kind] = dict(bytes=total, us_at_8TBps=round(1e6 * total / HBM_BYTES_PER_S, 2), fraction_of_roofline=round(1e6 * total / HBM_BYTES_PER_S / t, 4),
                              achieved_TBps=round(total / t / 1e6, 3))
        rec["records"][name] = dict(draw=dict(draw._asdict()), ksize=tables.ksize, table_bytes=int(tables.host.nbytes), times=times, bytes=nbytes,
                                    roofline=roof, host_route=host_name, bitwise=equal)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
