#!/usr/bin/env python3
"""Timing of one training step of the detector (``RaCFormer.forward_train`` + ``backward``) at the f8 shapes, B = 1: 8 frames x 6
cameras of 3 x 256 x 704, a 128 x 128 BEV grid, 900 queries with query denoising.  Random weights, ``synthetic`` inputs.  Needs the GPU.

    python tools/detector_train_bench.py [--out profiles/detector_train_f8.json] [--reps 5]

Device-event times in microseconds, medians with the 10th / 90th percentiles.  Two groups:
  step          the parts of one step, each bracketed by events inside the same step (the step is the detector's own code path
                written out: tests/detector_train_ref.py does the same for the tests): augmentation (``rac_image_aug_fwd``), backbone,
                necks, view transformer + DepthNet (frame 0 training, frames 1 .. T-1 eval), radar, head, loss, backward; and the whole
                ``forward_train`` + ``backward`` call
  augmentation  the one launch (parameter table on the device beforehand; and with the table built and uploaded inside the call, as
                the detector does) against the torch route of the same classes on the same drawn parameters (device float32 tensors
                both), with the launch's bytes (three planes in, three out) over the 8 TB/s roofline
Nothing is asserted.  Every figure in the record is measured by this run."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from detector_bench import CFG, DEV, PC, f8_model, frame, timed, window  # noqa: E402
from racformer_amd import RaCFormer, image_aug, synthetic as syn  # noqa: E402
from racformer_amd.detector import library_deterministic, pad_multiple  # noqa: E402

PEAK_BYTES_PER_S = 8.0e12
PARTS = ("augmentation", "backbone", "necks", "view_transformer_depthnet", "radar", "head", "loss", "backward")


def train_model():
    """f8_model() with the training entries of configs/racformer_r50_nuimg_704x256_f8.py:108-201"""
    m = f8_model()
    m["stop_prev_grad"] = 0
    m["pts_bbox_head"].update(
        query_denoising=True, query_denoising_groups=10, code_weights=[2.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], sync_cls_avg_factor=True,
        loss_cls=dict(type='FocalLoss', use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0),
        loss_bbox=dict(type='L1Loss', loss_weight=0.25), loss_iou=dict(type='GIoULoss', loss_weight=0.0))
    m["train_cfg"] = dict(pts=dict(
        grid_size=[512, 512, 1], voxel_size=[0.2, 0.2, 8], point_cloud_range=PC, out_size_factor=4,
        assigner=dict(type='PolarHungarianAssigner3D', cls_cost=dict(type='FocalLossCost', weight=2.0),
                      reg_cost=dict(type='BBox3DL1Cost', weight=0.25), theta_cost=dict(type='ThetaL1Cost', weight=3.0),
                      iou_cost=dict(type='IoUCost', weight=0.0))))
    return m


def ground_truth(n=30, seed=5):
    g = torch.Generator().manual_seed(seed)
    box = torch.cat([torch.rand(n, 2, generator=g) * 80 - 40, torch.rand(n, 1, generator=g) - 1, torch.rand(n, 3, generator=g) * 3 + 0.5,
                     torch.rand(n, 3, generator=g) - 0.5], dim=1)
    H, W = CFG.image_hw
    lidar = syn.make_lss_depth_inputs(n_maps=CFG.num_cams, input_hw=(H, W), lidar_density=0.1, seed=900)["lidar_depth"]
    return box, torch.arange(n) % 10, lidar[None].to(DEV)


class Marks:
    def __init__(self):
        self.ev = []

    def mark(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.ev.append(e)

    def spans(self):
        return [1e3 * a.elapsed_time(b) for a, b in zip(self.ev[:-1], self.ev[1:])]


def staged_step(det, a, gt, marks):
    """One step with an event between the parts: ``RaCFormer._extract_feat_train`` and ``forward_pts_train`` written out."""
    img, points, radar_depth, radar_rcs, metas = a
    box, labels, gt_depth = gt
    B, NT, C, H, W = img.shape
    N, T = det.num_cams, NT // det.num_cams
    marks.mark()
    x = img.reshape(B * NT, C, H, W).float()
    photo = det.color_aug.draw(B * NT)
    div = det.data_aug["img_pad_cfg"]["size_divisor"]
    for m in metas:
        m["img_shape"] = m["ori_shape"] = [(H, W, C)] * NT
    dm = pad_multiple(radar_depth.reshape(B * NT, 1, H, W).float(), metas, size_divisor=div)
    rm = pad_multiple(radar_rcs.reshape(B * NT, 1, H, W), metas, size_divisor=div)
    Hp, Wp = dm.shape[-2:]
    grid = det.grid_mask.draw(Hp)
    x = image_aug.prepare_images(x, photo, det.img_backbone.input_norm, div, grid)
    dm, rm = dm.reshape(B, N, T, Hp, Wp), rm.reshape(B, N, T, Hp, Wp)
    for m in metas:
        m.update(input_shape=x.shape[-2:])
    marks.mark()                                            # augmentation
    keep = det.img_backbone.input_norm
    try:
        det.img_backbone.input_norm = None
        stages = det.img_backbone(x)
    finally:
        det.img_backbone.input_norm = keep
    marks.mark()                                            # backbone
    fpn = det.img_neck(stages)
    lss = det.img_lss_neck(stages[-det.num_lss_fpn:])
    lss = lss[0] if isinstance(lss, (list, tuple)) else lss
    marks.mark()                                            # necks
    lss5 = lss.view(B, NT, *lss.shape[1:])
    vt = det.img_lss_view_transformer
    mlp = vt.get_mlp_input(metas)
    bevs, depths = [], []
    for i in range(T):
        mi = [dict(lidar2img=m["lidar2img"][i * N:(i + 1) * N], img_shape=m["img_shape"][i * N:(i + 1) * N]) for m in metas]
        call = lambda: vt(lss5[:, i * N:(i + 1) * N], dm[:, :, i], rm[:, :, i], mi, mlp[:, i * N:(i + 1) * N])     # noqa: E731
        if i == 0:
            with library_deterministic():
                bev, depth = call()
        else:
            with torch.no_grad(), det._branches_eval():
                bev, depth = call()
        bevs.append(bev)
        depths.append(depth)
    marks.mark()                                            # view transformer + DepthNet
    radars = []
    for i in range(T):
        if i == 0:
            radars.append(det.extract_pts_feat(points[i]))
        else:
            with torch.no_grad(), det._branches_eval():
                radars.append(det.extract_pts_feat(points[i]))
    marks.mark()                                            # radar
    metas[0]["gt_bboxes_3d"], metas[0]["gt_labels_3d"] = box, labels
    det.pts_bbox_head.transformer.decoder.pregrouped = False
    outs = det.pts_bbox_head([f.view(B, NT, *f.shape[1:]) for f in fpn], torch.stack(bevs, 1), torch.stack(radars, 1), metas)
    marks.mark()                                            # head
    losses = dict(loss_depth=vt.get_depth_loss(gt_depth, depths[0]))
    losses.update(det.pts_bbox_head.loss([box], [labels], outs))
    total = sum(losses.values())
    marks.mark()                                            # loss
    total.backward()
    marks.mark()                                            # backward
    return losses


def summary(samples):
    t = sorted(samples)
    return dict(median=round(statistics.median(t), 1), p10=round(t[len(t) // 10], 1), p90=round(t[(9 * len(t)) // 10], 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detector_train_f8.json"))
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    torch.manual_seed(0)
    np.random.seed(0)
    det = RaCFormer(**train_model())
    syn.fill_params(det.pts_bbox_head.transformer, 1)
    det = det.to(DEV)
    det.fused_grad = True
    det.train()
    T, N = CFG.num_frames, CFG.num_cams
    frames = [frame(f) for f in range(T)]
    gt = ground_truth()
    rec = dict(shape=dict(batch=1, frames=T, cams=N, image=list(CFG.image_hw), bev=list(CFG.bev_hw), queries=CFG.num_query, gt_boxes=int(gt[0].shape[0])),
               unit="us", measured="every figure is a device-event time measured by this run", device=torch.cuda.get_device_name(0))

    # ---- the step, part by part
    spans = {p: [] for p in PARTS}
    for r in range(2 + args.reps):
        det.zero_grad(set_to_none=True)
        marks = Marks()
        losses = staged_step(det, window(frames, list(range(T - 1, -1, -1))), gt, marks)
        torch.cuda.synchronize()
        if r >= 2:                                          # (two warm-up steps: weight packs, kernel attributes, the library's plans)
            for p, v in zip(PARTS, marks.spans()):
                spans[p].append(v)
    rec["step"] = {p: summary(v) for p, v in spans.items()}
    rec["step"]["sum_of_parts"] = round(sum(rec["step"][p]["median"] for p in PARTS), 1)
    rec["losses_last_step"] = {k: float(v) for k, v in losses.items()}

    def whole():
        det.zero_grad(set_to_none=True)
        img, points, depth, rcs, metas = window(frames, list(range(T - 1, -1, -1)))
        out = det.forward_train(img_metas=metas, gt_bboxes_3d=[gt[0]], gt_labels_3d=[gt[1]], gt_depth=gt[2], img=img, radar_points=points,
                                radar_depth=depth, radar_rcs=rcs)
        sum(out.values()).backward()

    rec["step"]["forward_train_backward"] = timed(dict(call=whole), args.reps, warmup=1)["call"]
    det.zero_grad(set_to_none=True)

    # ---- the augmentation launch against the torch route
    H, W = CFG.image_hw
    x = torch.cat([f[0] for f in frames]).float().contiguous()
    n = x.shape[0]
    photo = det.color_aug.draw(n)
    grid = None
    while grid is None:
        grid = det.grid_mask.draw(H)
    norm, div = det.img_backbone.input_norm, det.data_aug["img_pad_cfg"]["size_divisor"]
    Hp, Wp = image_aug.padded_size(H, W, div)
    with torch.no_grad():
        table = image_aug.device_table(n, photo, norm, x.device)
        aug = timed(dict(rac_image_aug_fwd=lambda: image_aug.image_aug_fwd(x, photo, norm, div, grid, table=table),
                         rac_image_aug_fwd_with_table_upload=lambda: image_aug.image_aug_fwd(x, photo, norm, div, grid),
                         torch_route=lambda: image_aug.prepare_images_torch(x, photo, norm, div, grid)), max(args.reps, 20))
        diff = float((image_aug.image_aug_fwd(x, photo, norm, div, grid) - image_aug.prepare_images_torch(x, photo, norm, div, grid)).abs().max())
    nbytes = 4 * 3 * n * (H * W + Hp * Wp)
    floor_us = 1e6 * nbytes / PEAK_BYTES_PER_S
    rec["augmentation"] = dict(images=n, bytes=nbytes, roofline_us_at_8TBps=round(floor_us, 1), **aug,
                               fraction_of_roofline=round(floor_us / aug["rac_image_aug_fwd"]["median"], 3),
                               speedup_over_torch_route=round(aug["torch_route"]["median"] / aug["rac_image_aug_fwd"]["median"], 1),
                               max_abs_difference_to_torch_route=diff)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
