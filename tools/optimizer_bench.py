#!/usr/bin/env python3
"""Timing of the optimiser step (``racformer_amd.optim.FusedAdamW`` -> ``rac_adamw_step``) on the f8 detector's trainable set, against
the library's routes.  Random weights, random gradients.  Needs the GPU.

    python tools/optimizer_bench.py [--out profiles/optimizer_f8.json] [--reps 30]

Device-event times in microseconds, medians with the 10th / 90th percentiles, the routes alternating inside one loop.  Groups:
  parameters    what the set is: tensors, elements, size range, tensors whose size is no multiple of 4, tensors of at most 64 elements,
                frozen elements, chunks
  fused_adamw   the three launches apart (sum of squares, finish, update), together (``launch``: the C entry alone, tables in place),
                and ``step()`` as a user calls it (signature walk, hyper check, launches, version bump); the bytes a step has to move
                (4 per element for the norm; 16 read and 12 written per element for the update) over the 8 TB/s roofline
  library       ``clip_grad_norm_(foreach=True)`` + ``torch.optim.AdamW(foreach=True).step()``, and the same with ``fused=True``, each
                on its own copy of the parameters (the clip rescales its gradients in place, so from the second repetition on they lie
                below the threshold and the coefficient is clamped to 1: the launches are the same)
  launches      device kernels per step of each route, counted by torch's profiler in a run of its own (None where the profiler
                gave nothing)
  train_step    one whole ``optim.train_step`` of the detector at f8, B = 1 with each optimiser (for the library routes:
                ``zero_grad``, forward, ``parse_losses``, backward, ``clip_grad_norm_``, ``step``), the three taking turns on the same
                detector inside one loop; and how often FusedAdamW rebuilt its device tables / re-sent the gradient pointers
Nothing is asserted and no ratio is fixed.  Every figure in the record is measured by this run."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from detector_bench import CFG, DEV, frame, timed, window  # noqa: E402
from detector_train_bench import ground_truth, train_model  # noqa: E402
from racformer_amd import RaCFormer, _lib, optim, synthetic as syn  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
RECIPE = dict(type='AdamW', lr=4e-4, weight_decay=0.01, grad_clip=dict(max_norm=35, norm_type=2),
              paramwise_cfg=dict(custom_keys={'img_backbone': dict(lr_mult=0.1), 'sampling_offset': dict(lr_mult=0.1)}))


class Named(torch.nn.Module):
    """a list of (name, parameter) as the module ``build_optimizer`` walks"""

    def __init__(self, ps):
        super().__init__()
        self._ps = ps

    def named_parameters(self, *a, **k):
        return iter(self._ps)


def library_optimizer(named, **kw):
    """torch.optim.AdamW with the recipe's per-parameter groups (``build_optimizer``'s, so the three routes do the same arithmetic)"""
    groups = [{k: v for k, v in g.items() if k in ("params", "lr", "weight_decay")} for g in optim.build_optimizer(Named(named), RECIPE).param_groups]
    return torch.optim.AdamW(groups, lr=RECIPE["lr"], weight_decay=RECIPE["weight_decay"], **kw)


def kernel_launches(fn):
    """device kernels of one call, from torch's profiler; None if it recorded none"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        # (on the device timeline the profiler also lists its own "Optimizer.step#..." annotation: not a launch)
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                 and "memset" not in e.name.lower() and not e.name.startswith("Optimizer.")]
        if not names:
            return None
        return dict(count=len(names), names=names) if len(names) <= 8 else dict(count=len(names), distinct=len(set(names)))
    except Exception as exc:        # (a profiler that cannot start is not this tool's subject)
        print(f"profiler: {exc!r}")
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optimizer_f8.json"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step-reps", type=int, default=9)
    args = ap.parse_args()
    torch.manual_seed(0)
    np.random.seed(0)
    det = RaCFormer(**train_model())
    syn.fill_params(det.pts_bbox_head.transformer, 1)
    det = det.to(DEV)
    det.fused_grad = True
    det.train()
    named = [(n, p) for n, p in det.named_parameters()]
    train = [(n, p) for n, p in named if p.requires_grad]
    sizes = [p.numel() for _, p in train]
    elements = sum(sizes)
    chunks = sum(-(-s // optim.CHUNK) for s in sizes)
    rec = dict(unit="us", measured="every figure is a device-event time measured by this run", device=torch.cuda.get_device_name(0),
               parameters=dict(tensors=len(named), trainable_tensors=len(train), trainable_elements=elements, smallest=min(sizes),
                               largest=max(sizes), not_multiple_of_4=sum(1 for s in sizes if s % 4), at_most_64=sum(1 for s in sizes if s <= 64),
                               frozen_elements=sum(p.numel() for _, p in named if not p.requires_grad), chunk=optim.CHUNK, chunks=chunks))

    # ---- the optimiser step alone: three copies of the trainable set, the same random gradients
    g = torch.Generator(device=DEV).manual_seed(1)
    grads = [torch.randn(p.shape, generator=g, device=DEV) * 1e-3 for _, p in train]

    def copy_set():
        ps = [(n, torch.nn.Parameter(p.detach().clone())) for n, p in train]
        for (_, p), gr in zip(ps, grads):
            p.grad = gr.clone()
        return ps

    ours_set, foreach_set, fused_set = copy_set(), copy_set(), copy_set()

    ours = optim.build_optimizer(Named(ours_set), RECIPE)
    ours.prepare()
    lib_foreach = library_optimizer(foreach_set, foreach=True)
    lib_fused = library_optimizer(fused_set, fused=True)

    def library(opt, ps, **kw):
        params = [p for _, p in ps]

        def run():
            torch.nn.utils.clip_grad_norm_(params, 35, 2, **kw)
            opt.step()
        return run

    routes = dict(
        sum_of_squares=lambda: ours.launch(_lib.OPT_NORM), finish=lambda: ours.launch(_lib.OPT_FINISH), update=lambda: ours.launch(_lib.OPT_UPDATE),
        launch=lambda: ours.launch(_lib.OPT_ALL), step=ours.step,
        library_foreach=library(lib_foreach, foreach_set, foreach=True), library_fused=library(lib_fused, fused_set, foreach=True))
    t = timed(routes, args.reps, warmup=3)
    norm_bytes, update_bytes = 4 * elements, 28 * elements
    floor = 1e6 * (norm_bytes + update_bytes) / PEAK_BYTES_PER_S
    rec["fused_adamw"] = dict(
        {k: t[k] for k in ("sum_of_squares", "finish", "update", "launch", "step")}, bytes_norm=norm_bytes, bytes_update=update_bytes,
        roofline_us_at_8TBps=round(floor, 1), launch_fraction_of_roofline=round(floor / t["launch"]["median"], 3),
        sum_of_squares_fraction_of_roofline=round(1e6 * norm_bytes / PEAK_BYTES_PER_S / t["sum_of_squares"]["median"], 3),
        update_fraction_of_roofline=round(1e6 * update_bytes / PEAK_BYTES_PER_S / t["update"]["median"], 3))
    rec["library"] = dict(clip_foreach_adamw_foreach=t["library_foreach"], clip_foreach_adamw_fused=t["library_fused"])
    rec["launches"] = dict(fused_adamw_step=kernel_launches(routes["step"]), clip_foreach_adamw_foreach=kernel_launches(routes["library_foreach"]),
                           clip_foreach_adamw_fused=kernel_launches(routes["library_fused"]))
    del ours, lib_foreach, lib_fused, ours_set, foreach_set, fused_set, grads, routes
    torch.cuda.empty_cache()

    # ---- one whole training step of the detector with each optimiser
    T = CFG.num_frames
    frames = [frame(f) for f in range(T)]
    gt = ground_truth()

    def data():
        img, points, depth, rcs, metas = window(frames, list(range(T - 1, -1, -1)))
        return dict(img_metas=metas, gt_bboxes_3d=[gt[0]], gt_labels_3d=[gt[1]], gt_depth=gt[2], img=img, radar_points=points, radar_depth=depth,
                    radar_rcs=rcs)

    # The three optimisers take turns on the same detector inside one loop (each keeps its own moments; the weights wander, the work
    # of a step does not depend on them), so that drift of the machine over the run falls on all three alike.
    ours = optim.build_optimizer(det, RECIPE)

    def library_step(opt):
        def call():
            opt.zero_grad(set_to_none=True)
            loss, _ = optim.parse_losses(det(return_loss=True, **data()))
            loss.backward()
            torch.nn.utils.clip_grad_norm_([p for p in det.parameters() if p.grad is not None], 35, 2, foreach=True)
            opt.step()
        return call

    rec["train_step"] = timed(dict(fused_adamw=lambda: optim.train_step(det, ours, **data()),
                                   clip_foreach_adamw_foreach=library_step(library_optimizer(named, foreach=True)),
                                   clip_foreach_adamw_fused=library_step(library_optimizer(named, fused=True))), args.step_reps, warmup=2)
    # how often the tables were rebuilt, and how often set_to_none moved the gradient buffers so that their pointers were sent again
    rec["train_step"]["fused_adamw"].update(steps=args.step_reps + 2, table_builds=ours.table_builds, table_uploads=ours.table_uploads)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
