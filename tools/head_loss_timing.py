#!/usr/bin/env python3
"""RaCFormer_head.loss (fused: rac_match_cost_fwd + rac_lsap_fwd + rac_det_loss_fwd for all layers and samples, rac_det_loss_fwd
for the denoising rows) against loss_unfused (the reference's route: per layer and sample a torch cost matrix, a copy to the host,
the host solver, scattered targets, FocalLoss / L1Loss) on the same tensors in one process.
Shapes: the f8 head -- 6 layers, 900 queries, 10 classes, 10 denoising groups -- with B = 1 and 4 samples of about 40 and about 200
boxes each.  The unfused route stalls the host 6 * B times a step, so both routes are timed by the host clock between two device
synchronisations (what a training step waits for): after a warm-up, alternating batches until each route has --window-ms;
medians per call.  The three kernels alone are timed between device events, and the solver's Dijkstra step counts are recorded.

    python tools/head_loss_timing.py [--out profiles/head_loss_f8.json]
"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from msmv_v2_timing import summary, time_pair  # noqa: E402
from racformer_amd.fused import det_loss_fused, lsap_fused, match_cost_fused  # noqa: E402
from racformer_amd.head import RaCFormer_head  # noqa: E402

L, Q, C, GROUPS = 6, 900, 10, 10
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
CODE_WEIGHTS = [2.0, 2.0] + [1.0] * 8
ASSIGNER = dict(type="PolarHungarianAssigner3D", cls_cost=dict(type="FocalLossCost", weight=2.0),
                reg_cost=dict(type="BBox3DL1Cost", weight=0.25), theta_cost=dict(type="ThetaL1Cost", weight=3.0),
                iou_cost=dict(type="IoUCost", weight=0.0))


def make_head(dev):
    return RaCFormer_head(num_classes=C, in_channels=256, num_query=Q, num_clusters=5, code_size=10, code_weights=CODE_WEIGHTS,
                          query_denoising=True, query_denoising_groups=GROUPS, sync_cls_avg_factor=True, transformer=None,
                          bbox_coder=dict(type="NMSFreeCoder", post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], pc_range=PC_RANGE,
                                          max_num=300, score_threshold=0.05, num_classes=C),
                          loss_cls=dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0),
                          loss_bbox=dict(type="L1Loss", loss_weight=0.25), loss_iou=dict(type="GIoULoss", loss_weight=0.0),
                          train_cfg=dict(assigner=ASSIGNER)).to(dev).train()


def boxes_like_outputs(rng, shape):
    b = np.zeros(shape + (10,), np.float32)
    b[..., 0:2] = rng.uniform(-50, 50, shape + (2,))
    b[..., 2:4] = rng.uniform(-0.7, 1.7, shape + (2,))
    b[..., 4] = rng.uniform(-2, 1, shape)
    b[..., 5] = rng.uniform(-0.7, 1.7, shape)
    ang = rng.uniform(-np.pi, np.pi, shape)
    b[..., 6], b[..., 7] = np.sin(ang), np.cos(ang)
    b[..., 8:10] = rng.uniform(-3, 3, shape + (2,))
    return b


def make_case(B, G, dev, seed):
    rng = np.random.default_rng(seed)
    counts = [int(G + rng.integers(-G // 8, G // 8 + 1)) for _ in range(B)]
    gts, labels = [], []
    for n in counts:
        t = np.zeros((n, 9), np.float32)
        t[:, 0:2] = rng.uniform(-48, 48, (n, 2))
        t[:, 2] = rng.uniform(-2, 1, n)
        t[:, 3:6] = rng.uniform(0.5, 5, (n, 3))
        t[:, 6] = rng.uniform(-np.pi, np.pi, n)
        t[:, 7:9] = rng.uniform(-3, 3, (n, 2))
        gts.append(torch.from_numpy(t).to(dev))
        labels.append(torch.from_numpy(rng.integers(0, C, n)).to(dev))
    single, total = max(counts), sum(counts)
    pad = single * GROUPS
    batch_idx = torch.cat([torch.full((n,), i, dtype=torch.long) for i, n in enumerate(counts)]).to(dev)
    within = torch.cat([torch.arange(n) for n in counts])
    md = {"known_indice": torch.arange(total, device=dev).repeat(GROUPS), "batch_idx": batch_idx,
          "map_known_indice": torch.cat([within + single * i for i in range(GROUPS)]).to(dev),
          "known_lbs_bboxes": (torch.cat(labels).repeat(GROUPS), torch.cat(gts).repeat(GROUPS, 1)), "pad_size": pad}
    leaves = {"all_cls_scores": torch.from_numpy(rng.normal(-2, 1.5, (L, B, Q, C)).astype(np.float32)).to(dev).requires_grad_(),
              "all_bbox_preds": torch.from_numpy(boxes_like_outputs(rng, (L, B, Q))).to(dev).requires_grad_(),
              "dn_cls": torch.from_numpy(rng.normal(-2, 1.5, (L, B, pad, C)).astype(np.float32)).to(dev).requires_grad_(),
              "dn_box": torch.from_numpy(boxes_like_outputs(rng, (L, B, pad))).to(dev).requires_grad_()}
    md["output_known_lbs_bboxes"] = (leaves["dn_cls"], leaves["dn_box"])
    preds = {"all_cls_scores": leaves["all_cls_scores"], "all_bbox_preds": leaves["all_bbox_preds"], "enc_cls_scores": None,
             "enc_bbox_preds": None, "dn_mask_dict": md}
    return counts, gts, labels, preds, leaves


def host_clock_pair(fn_a, fn_b, batch, window_ms, warmup):
    for _ in range(warmup):
        fn_a()
        fn_b()
    res, total = {"a": [], "b": []}, {"a": 0.0, "b": 0.0}
    while min(total.values()) < window_ms:
        for key, fn in (("a", fn_a), ("b", fn_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(batch):
                fn()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            total[key] += ms
            res[key].append(ms / batch)
    return res, total


def one_shape(B, G, args):
    dev = "cuda:0"
    head = make_head(dev)
    counts, gts, labels, preds, leaves = make_case(B, G, dev, seed=B * 1000 + G)
    lv = list(leaves.values())

    def fused_fwd():
        with torch.no_grad():
            head.loss(gts, labels, preds)

    def unfused_fwd():
        with torch.no_grad():
            head.loss_unfused(gts, labels, preds)

    def fused_step():
        torch.autograd.grad(sum(head.loss(gts, labels, preds).values()), lv)

    def unfused_step():
        torch.autograd.grad(sum(head.loss_unfused(gts, labels, preds).values()), lv)

    a, b = head.loss(gts, labels, preds), head.loss_unfused(gts, labels, preds)
    worst = max(abs(float(a[k].detach()) - float(b[k].detach())) / max(abs(float(b[k].detach())), 1e-12) for k in a)
    rec = {"shape": {"layers": L, "B": B, "Q": Q, "classes": C, "boxes_per_sample": counts, "denoising_groups": GROUPS,
                     "denoising_rows_per_layer": GROUPS * sum(counts)},
           "max_rel_diff_fused_vs_unfused_over_the_24_keys": worst}
    res, total = host_clock_pair(fused_fwd, unfused_fwd, args.batch, args.window_ms, args.warmup)
    rec["loss_forward_fused"], rec["loss_forward_unfused"] = summary(res["a"], total["a"]), summary(res["b"], total["b"])
    res, total = host_clock_pair(fused_step, unfused_step, args.batch, args.window_ms, args.warmup)
    rec["loss_forward_backward_fused"], rec["loss_forward_backward_unfused"] = summary(res["a"], total["a"]), summary(res["b"], total["b"])
    rec["unfused_over_fused_forward_median"] = round(rec["loss_forward_unfused"]["median_us"] / rec["loss_forward_fused"]["median_us"], 2)
    rec["unfused_over_fused_step_median"] = round(rec["loss_forward_backward_unfused"]["median_us"] / rec["loss_forward_backward_fused"]["median_us"], 2)

    # the kernels alone, between device events
    cls, box = leaves["all_cls_scores"].detach(), leaves["all_bbox_preds"].detach()
    table, lab32 = torch.cat(gts), torch.cat(labels).to(torch.int32)
    cw = head.code_weights.detach()
    cost = match_cost_fused(cls, box, table, lab32, counts, cw, 2.0, 0.25, 3.0)
    _, assigned, _, _, steps = lsap_fused(cost, counts, L, Q, with_steps=True)
    rows = (cls.view(L, B * Q, C), box.view(L, B * Q, 10), assigned.view(L, B * Q))
    res, total = time_pair(lambda: match_cost_fused(cls, box, table, lab32, counts, cw, 2.0, 0.25, 3.0, out=cost),
                           lambda: lsap_fused(cost, counts, L, Q), args.batch, args.window_ms / 2, args.warmup)
    rec["rac_match_cost_fwd"], rec["rac_lsap_fwd"] = summary(res["a"], total["a"]), summary(res["b"], total["b"])
    res, total = time_pair(lambda: det_loss_fused(*rows, table, lab32, cw), lambda: lsap_fused(cost, counts, L, Q), args.batch,
                           args.window_ms / 2, args.warmup)
    rec["rac_det_loss_fwd_matching_rows"] = summary(res["a"], total["a"])
    st = steps.cpu().view(L, B)
    rec["lsap_dijkstra_steps"] = {"per_problem": st.tolist(), "max": int(st.max()),
                                  "worst_case_bound_G(G+1)/2": [n * (n + 1) // 2 for n in counts]}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=400.0)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    rec = {"what": "RaCFormer_head.loss (fused HIP route) against loss_unfused (per layer and sample: torch cost, copy to the host, host "
                   "solver, torch losses) on the same tensors; host clock between device synchronisations, alternating batches, medians "
                   "(tools/head_loss_timing.py); the three kernels alone between device events",
           "batch": args.batch, "warmup_calls_each": args.warmup, "window_ms": args.window_ms, "device": torch.cuda.get_device_name(0)}
    for B in (1, 4):
        for G in (40, 200):
            rec[f"B{B}_G{G}"] = one_shape(B, G, args)
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
