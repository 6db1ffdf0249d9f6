#!/usr/bin/env python3
"""Timing of the detector (racformer_amd/detector.py) at the f8 shapes: 8 frames x 6 cameras of 3 x 256 x 704, a 128 x 128 BEV grid,
900 queries.  Random weights, ``synthetic`` inputs.  Needs the GPU.

    python tools/detector_bench.py [--out profiles/detector_f8.json] [--reps 20]

Device-event times in microseconds, medians with the 10th / 90th percentiles; inside a group the functions alternate in every
repetition after a warm-up (tools/resnet_bench.py's scheme).  Three groups:
  offline     the stages of ``simple_test_offline``, each on the stage before's own output: backbone (48 images), necks
              (``FPN.forward_pregrouped`` + ``CustomFPN``), the per-frame view-transformer loop, the per-frame radar loop, decoder +
              decode (``pts_bbox_head`` + ``get_bboxes``); and the whole call
  streaming   the steady-state step of ``simple_test_online``: the front end on one frame (``extract_feat``, T = 1), the slot copy,
              the gather launch, ``CapturedStep.replay`` + ``get_bboxes``; and the whole call with one new frame per step; the
              ``*_built_maps`` entries are the same front end and the same whole call with ``radar_depth=None, radar_rcs=None`` (the
              maps made on the device from the frame's cloud, racformer_amd/point_maps.py)
  gather      ``rac_frames_gather`` of the window beside ``Tensor.copy_`` of the same bytes (T consecutive slots per kind, six calls)
Nothing is asserted.  Every figure in the record is measured by this run; ``expectation`` repeats what DESIGN.md derived beforehand."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from racformer_amd import RaCFormer, fused, synthetic as syn  # noqa: E402

DEV = "cuda:0"
CFG = syn.F8
PC = list(syn.PC_RANGE)
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def f8_model():
    """configs/racformer_r50_nuimg_704x256_f8.py:108-201 without the training-only entries"""
    return dict(
        data_aug=dict(img_color_aug=True, img_norm_cfg=NORM, img_pad_cfg=dict(size_divisor=32)),
        img_backbone=dict(type='ResNet', depth=50, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                          norm_cfg=dict(type='BN2d', requires_grad=True), norm_eval=True, style='pytorch', with_cp=True),
        img_neck=dict(type='FPN', in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=4),
        img_lss_neck=dict(type='CustomFPN', in_channels=[1024, 2048], out_channels=256, num_outs=1, start_level=0, out_ids=[0]),
        img_lss_view_transformer=dict(type='LSSViewTransformerBEVDepth_racformer',
                                      grid_config=dict(x=[-51.2, 51.2, 0.8], y=[-51.2, 51.2, 0.8], z=[-5, 3, 8], depth=[1.0, 65.0, 96.0],
                                                       rcs=[-64, 64, 64]),
                                      input_size=(256, 704), in_channels=256, out_channels=256, depthnet_cfg=dict(use_dcn=False),
                                      downsample=16, loss_depth_weight=2.0),
        num_lss_fpn=2,
        radar_voxel_layer=dict(max_num_points=10, voxel_size=[0.8, 0.8, 8], max_voxels=(30000, 40000), point_cloud_range=PC, deterministic=False),
        radar_voxel_encoder=dict(type='PillarFeatureNet', in_channels=7, feat_channels=[64], with_distance=False, voxel_size=[0.8, 0.8, 8],
                                 norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01), legacy=False),
        radar_middle_encoder=dict(type='PointPillarsScatter', in_channels=64, output_shape=(128, 128)),
        pts_bbox_head=dict(type='RaCFormer_head', num_classes=10, num_clusters=6, in_channels=256, num_query=900, code_size=10,
                           transformer=dict(type='RaCFormerTransformer', **CFG.transformer_kwargs()),
                           bbox_coder=dict(type='NMSFreeCoder', post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0], pc_range=PC,
                                           max_num=300, voxel_size=[0.2, 0.2, 8], score_threshold=0.05, num_classes=10)),
        num_cams=6)


def timed(fns, reps, warmup=3):
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
    out = {}
    for k, v in ev.items():
        t = sorted(1e3 * a.elapsed_time(b) for a, b in v)
        out[k] = dict(median=round(statistics.median(t), 1), p10=round(t[len(t) // 10], 1), p90=round(t[(9 * len(t)) // 10], 1))
    return out


def frame(fid):
    H, W = CFG.image_hw
    img = torch.from_numpy(syn.rng_uniform(9000 + fid, (6, 3, H, W), 0.0, 255.0))
    maps = syn.make_lss_depth_inputs(n_maps=6, input_hw=(H, W), seed=70 + fid)
    cloud = syn.make_radar_points(1, 1500, seed=40 + fid)[0]
    return img.to(DEV), maps["radar_depth"].unsqueeze(1).to(DEV), maps["radar_rcs"].unsqueeze(1).to(DEV), cloud.to(DEV)


def window(frames, fids):
    """the inputs of one call for the frame ids ``fids`` (newest first); the data cycles over the prepared frames"""
    fr = [frames[f % len(frames)] for f in fids]
    return (torch.cat([f[0] for f in fr])[None], [[f[3]] for f in fr], torch.cat([f[1] for f in fr])[None],
            torch.cat([f[2] for f in fr])[None], metas_of(fids))


def metas_of(fids):
    """fresh metas (a call rewrites them): host lists only"""
    metas = syn.make_img_metas(syn.replace(CFG, num_frames=len(fids)))
    metas[0]["filename"] = [f"frame{f:04d}_cam{n}.jpg" for f in fids for n in range(6)]
    return metas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detector_f8.json"))
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    torch.manual_seed(0)
    det = RaCFormer(**f8_model())
    syn.fill_params(det.pts_bbox_head.transformer, 1)
    det = det.to(DEV).eval()
    T, N = CFG.num_frames, CFG.num_cams
    frames = [frame(f) for f in range(12)]
    rec = dict(shape=dict(frames=T, cams=N, image=list(CFG.image_hw), bev=list(CFG.bev_hw), queries=CFG.num_query), unit="us",
               measured="every figure under offline / streaming / gather is a device-event time measured by this run",
               device=torch.cuda.get_device_name(0))

    # ---- offline, stage by stage
    img, points, depth, rcs, metas = window(frames, list(range(T - 1, -1, -1)))
    x = img.view(T * N, 3, *CFG.image_hw)
    vt, head = det.img_lss_view_transformer, det.pts_bbox_head
    with torch.no_grad():
        stages = det.img_backbone(x)
        lss = det.img_lss_neck(stages[-2:]).view(1, T * N, 256, 16, 44)
        H, W = CFG.image_hw
        dm, rm = depth.view(1, N, T, H, W), rcs.view(1, N, T, H, W)
        all_fids = list(range(T - 1, -1, -1))
        feats, bev, radar, _ = det.extract_feat(img, points, depth, rcs, metas_of(all_fids))

        def lss_loop():
            mlp = vt.get_mlp_input(metas)
            for i in range(T):
                m = [dict(lidar2img=metas[0]["lidar2img"][i * N:(i + 1) * N])]
                vt(lss[:, i * N:(i + 1) * N], dm[:, :, i], rm[:, :, i], m, mlp[:, i * N:(i + 1) * N])

        def offline():
            det.simple_test_offline(metas_of(all_fids), img, False, points, depth, rcs)

        def decoder():
            m = metas_of(all_fids)
            head.get_bboxes(head(list(feats), bev, radar, m), m[0])

        rec["offline"] = timed(dict(
            backbone=lambda: det.img_backbone(x),
            necks=lambda: (det.img_neck.forward_pregrouped(list(stages)), det.img_lss_neck(stages[-2:])),
            lss_loop=lss_loop,
            radar_loop=lambda: [det.extract_pts_feat(p) for p in points],
            decoder_and_decode=decoder,
            whole=offline), args.reps)

    # ---- streaming: warm the memory and the captured step, then the steady state
    det.reset_memory()
    step = [0]

    def online(built_maps=False):
        s = step[0] = step[0] + 1
        w = window(frames, [max(s - t, 0) for t in range(T)])                             # one new key per step
        if built_maps:                          # the radar maps made on the device from the new frame's cloud
            return det.simple_test_online(w[4], w[0], False, w[1], None, None)
        return det.simple_test_online(w[4], w[0], False, w[1], w[2], w[3])

    for _ in range(T + 2):
        online()
    assert det._plan is not None and det.stats["computed"] == 1
    one = window(frames, [3])
    mem, win = det.memory, det._window
    slots = list(mem.slots.values())[-T:]
    with torch.no_grad():
        f1 = det.extract_feat(one[0], one[1], one[2], one[3], metas_of([3]))
        tensors = det._frame_tensors(f1[0], f1[1], f1[2])
        spare = mem.free[-1]
        big = metas_of(all_fids)

        def replay():
            outs, _ = det._plan.replay(img_metas=big)
            head.get_bboxes(outs, big[0])

        rec["streaming"] = timed(dict(
            front_end_one_frame=lambda: det.extract_feat(one[0], one[1], one[2], one[3], metas_of([3])),
            slot_copy=lambda: [r[spare].copy_(t) for r, t in zip(mem.rings, tensors)],
            gather=lambda: fused.frames_gather(mem.rings, win, slots),
            replay_and_decode=replay,
            whole=online,
            front_end_one_frame_built_maps=lambda: det.extract_feat(one[0], one[1], None, None, metas_of([3])),
            whole_built_maps=lambda: online(True)), args.reps)
        rec["streaming"]["memory"] = dict(slots=mem.n_slots, ring_bytes=sum(r.numel() * 4 for r in mem.rings),
                                          window_bytes=sum(w.numel() * 4 for w in win))

        # ---- the gather beside Tensor.copy_ of the same bytes
        flat = [w.view(T, -1) for w in win]
        rec["gather"] = timed(dict(
            rac_frames_gather=lambda: fused.frames_gather(mem.rings, win, slots),
            rac_frames_gather_identity=lambda: fused.frames_gather(mem.rings, win, list(range(T))),
            tensor_copy=lambda: [o.copy_(r[:T].view(T, -1)) for o, r in zip(flat, mem.rings)]), args.reps)
        rec["gather"]["bytes"] = rec["streaming"]["memory"]["window_bytes"]
        for k in ("rac_frames_gather", "rac_frames_gather_identity", "tensor_copy"):
            rec["gather"][k]["GBps_read_plus_write"] = round(2 * rec["gather"]["bytes"] / rec["gather"][k]["median"] / 1e3, 1)
    rec["expectation"] = "derived, not measured (DESIGN.md 3.21 and the README): about 1/8 of the offline front end plus the 4.3 ms decoder step"
    det.reset_memory()
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
