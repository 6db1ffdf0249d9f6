#!/usr/bin/env python3
"""Timing of the radar pillar branch (racformer_amd/radar_pillars.py) on the f8 shape: B = 1, T = 8 frames of 1500 radar points
(SURVEY.md 8d), 7 values a point, a 128 x 128 grid of 0.8 m pillars, 64 -> 64 -> 64 -> 256 channels.  Needs the GPU.

    python tools/radar_pillars_bench.py [--out profiles/radar_pillars_f8.json]

All times between device events on one stream after a warm-up, medians over --reps calls, the routes alternating inside every
repetition:
  stages    every launch group of the fused route alone (voxelize, pillar encode + scatter into the activation image, the three
            convolution layers), and the stages of the torch-ops route (fused=False: stable sort voxelization with its host
            round trips, nn.Linear / BatchNorm1d / max, indexed scatter, the library's Conv2d + BatchNorm2d + ReLU)
  total     points -> [B, T, 256, H, W], both routes, same device, same inputs
  last_layer  the 64 -> 256 layer on the direct kernel (rac_conv_direct_fwd, RAC_CD_F32_CF_RELU) against the LDS-staged kernel
            (rac_conv3x3_relu_cf_fwd, what the encoder uses; and rac_conv3x3_fwd, its channel-last form without the ReLU)
The pillar counts of the rig and the largest difference between the two routes' results go into the record.

    python tools/radar_pillars_bench.py --train [--out profiles/radar_pillars_grad_f8.json]

times the training route instead (``RadarPillarEncoder.fused_grad``, frame 0 only, B = 1 and B = 2 clouds): forward + backward of
the HIP route against the torch route on the same GPU (library convolution + nn.BatchNorm under autograd; once whole, once behind
its host-side voxelization), and every launch group of the HIP route alone.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from racformer_amd import radar_pillars as RP, synthetic as syn  # noqa: E402
from racformer_amd.fused import ConvImage, act_image  # noqa: E402


def timed(fns, reps, warmup=5):
    """{name: median ms}; the functions alternate inside every repetition"""
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
    return {k: round(statistics.median(a.elapsed_time(b) for a, b in v), 4) for k, v in ev.items()}


def train_record(args, dev, B):
    """Forward + backward of frame 0 in training mode (``RadarPillarEncoder.fused_grad``): the HIP route against the torch route
    (library convolution + nn.BatchNorm under autograd) on B clouds, and the HIP route's launch groups alone."""
    from racformer_amd import resnet
    clouds = [c.to(dev) for c in syn.make_radar_points(B, args.points, seed=31, edge_fraction=0.05)]
    torch.manual_seed(3)
    fused, loose = RP.RadarPillarEncoder().to(dev).train(), RP.RadarPillarEncoder(fused=False).to(dev).train()
    loose.load_state_dict(fused.state_dict())
    fused.fused_grad = loose.fused_grad = True
    gout = torch.randn(B, 256, *fused.radar_middle_encoder.output_shape, device=dev)

    def step(enc):
        for p in enc.parameters():
            p.grad = None
        enc.extract_pts_feat(clouds).backward(gout)

    step(fused), step(loose)
    named = dict(loose.named_parameters())
    agree = {k: float((p.grad - named[k].grad).abs().max() / named[k].grad.abs().max()) for k, p in fused.named_parameters()}

    # ---- the torch route behind its voxelization (which goes through the host)
    zeroed = [c.clone() for c in clouds]
    for c in zeroed:
        c[:, 2] = 0
    with torch.no_grad():
        tv, tn, tc = loose.radar_voxelize(zeroed)

    def torch_stack():
        for p in loose.parameters():
            p.grad = None
        feats = loose.radar_voxel_encoder.forward_torch(tv, tn, tc)
        loose.radar_bev_conv(loose.radar_middle_encoder(feats, tc, B)).backward(gout)

    # ---- the HIP route's launch groups
    vl, pfn = fused.radar_voxel_layer, fused.radar_voxel_encoder
    gx, gy, _ = vl.geom.grid
    pts, off = RP.pack_clouds(clouds, zero_z=True)
    pv = RP.voxelize_packed(pts, off, vl.geom, vl.max_num_points, vl.cap())
    counts = pv.counts.cpu().tolist()
    canvas, pfn_saved = pfn.train_fwd(pv, gy, gx)
    _, _, layers = fused.train_forward_hip(pts, off)
    groups = {
        "pack_clouds": lambda: RP.pack_clouds(clouds, zero_z=True, pinned=True),
        "voxelize": lambda: RP.voxelize_packed(pts, off, vl.geom, vl.max_num_points, vl.cap()),
        "pfn_train_fwd": lambda: pfn.train_fwd(pv, gy, gx),
        "pfn_train_bwd": lambda: pfn.train_bwd(pfn_saved, canvas),
    }
    for i, (x, z, y, mean, invstd) in enumerate(layers):
        bn = fused.radar_bev_conv[i].bn
        gz = RP.bn_train_bwd(y, z, y, mean, invstd, bn.weight)[2]
        tag = f"layer{i}_"
        groups.update({
            tag + "absmax_conv_fwd": lambda x=x, i=i: resnet.conv_fwd(x, fused.train_packs(i), None, 3, 1, relu=False),
            tag + "bn_stats": lambda z=z, bn=bn: RP.bn_train_stats(z, bn),
            tag + "bn_apply": lambda z=z, mean=mean, invstd=invstd, bn=bn: RP.bn_train_apply(z, mean, invstd, bn.weight, bn.bias),
            tag + "bn_bwd": lambda z=z, y=y, mean=mean, invstd=invstd, bn=bn: RP.bn_train_bwd(y, z, y, mean, invstd, bn.weight),
            tag + "conv_wgrad": lambda gz=gz, x=x: resnet.conv_wgrad(gz, x, 3, 1, bias=False),
            tag + "absmax_conv_dgrad": lambda gz=gz, x=x, i=i: resnet.conv_dgrad(gz, fused.train_packs(i, transposed=True), 3, 1,
                                                                                   x.shape[2:], mask=x if i else None),
        })
    total = timed({"hip_fwd_bwd": lambda: step(fused), "torch_fwd_bwd": lambda: step(loose), "torch_fwd_bwd_behind_voxelize": torch_stack},
                  args.reps)
    split = timed(groups, args.reps)
    top = max(split, key=split.get)
    return dict(B=B, pillars_per_cloud=counts, total=total, hip_launch_groups=split, hip_launch_groups_sum=round(sum(split.values()), 4),
                dominant_launch_group=top, dominant_share_of_groups=round(split[top] / sum(split.values()), 3),
                hip_faster_than_torch=total["hip_fwd_bwd"] < total["torch_fwd_bwd"],
                hip_faster_than_torch_behind_voxelize=total["hip_fwd_bwd"] < total["torch_fwd_bwd_behind_voxelize"],
                grad_max_rel_diff_hip_vs_torch=max(agree.values()))


def main_train(args, dev):
    enc = RP.RadarPillarEncoder()
    gx, gy, _ = enc.radar_voxel_layer.geom.grid
    rec = dict(shape=dict(frames="frame 0 only", points_per_cloud=args.points, width=7, grid=[gx, gy, 1], channels=[64, 64, 64, 256],
                          max_num_points=enc.radar_voxel_layer.max_num_points, max_voxels=enc.radar_voxel_layer.max_voxels[0]),
               device=torch.cuda.get_device_name(0), unit="ms, median of device-event times, forward + backward", reps=args.reps,
               runs=[train_record(args, dev, B) for B in (1, 2)])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--points", type=int, default=1500)
    ap.add_argument("--train", action="store_true", help="time forward + backward of the training route (B = 1 and 2, frame 0 only)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "radar_pillars_bench needs the MI355X"
    dev = torch.device("cuda:0")
    if args.out is None:
        args.out = os.path.join(ROOT, "build", "radar_pillars_grad_f8.json" if args.train else "radar_pillars_f8.json")
    if args.train:
        return main_train(args, dev)
    B, T = 1, args.frames
    clouds = [c.to(dev) for c in syn.make_radar_points(B * T, args.points, seed=31, edge_fraction=0.05)]
    frames = [[clouds[t]] for t in range(T)]
    torch.manual_seed(3)
    fused, loose = RP.RadarPillarEncoder().to(dev).eval(), RP.RadarPillarEncoder(fused=False).to(dev).eval()
    for m in fused.modules():
        if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
            m.running_mean.normal_(0, 0.3)
            m.running_var.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
    loose.load_state_dict(fused.state_dict())

    with torch.no_grad():
        a, b = fused(frames), loose(frames)
        agree = float((a - b).abs().max())
        top = float(b.abs().max())

        # ---- the fused route's launch groups
        vl, pfn = fused.radar_voxel_layer, fused.radar_voxel_encoder
        gx, gy, _ = vl.geom.grid
        n = B * T
        pts, off = RP.pack_clouds(clouds, zero_z=True)
        pv = RP.voxelize_packed(pts, off, vl.geom, vl.max_num_points, vl.cap())
        counts = pv.counts.cpu().tolist()
        convs = fused.packed_convs()
        img_a, img_b = act_image("bench_a", n, gy, gx, 64, dev), act_image("bench_b", n, gy, gx, 64, dev)
        s0 = (pv.amax,) + pfn.image_bound()
        s1 = RP.next_scale(s0, convs[0])
        s2 = RP.next_scale(s1, convs[1])
        out = torch.empty(n, 256, gy, gx, device=dev)
        canvas = torch.empty(n, 64, gy, gx, device=dev)

        # ---- the torch-ops route's stages
        zeroed = [c.clone() for c in clouds]
        for c in zeroed:
            c[:, 2] = 0
        tv, tn, tc = loose.radar_voxelize(zeroed)
        tf = loose.radar_voxel_encoder(tv, tn, tc)
        tcanvas = loose.radar_middle_encoder(tf, tc, n)

        stages = timed({
            "fused_pack_clouds": lambda: RP.pack_clouds(clouds, zero_z=True),
            "fused_voxelize": lambda: RP.voxelize_packed(pts, off, vl.geom, vl.max_num_points, vl.cap()),
            "fused_encode_scatter_image": lambda: pfn.encode(pv.voxels, pv.coors, pv.num_points, n, gy, gx, amax=pv.amax, image=img_a),
            "fused_encode_scatter_canvas": lambda: pfn.encode(pv.voxels, pv.coors, pv.num_points, n, gy, gx, canvas=canvas),
            "fused_conv0_64_64": lambda: RP.conv_bn_relu(convs[0], img_a, s0, n, gy, gx, out_img=img_b, out_scale=s1),
            "fused_conv1_64_64": lambda: RP.conv_bn_relu(convs[1], img_b, s1, n, gy, gx, out_img=img_a, out_scale=s2),
            "fused_conv2_64_256": lambda: RP.conv_bn_relu(convs[2], img_a, s2, n, gy, gx, out=out),
            "torch_voxelize": lambda: loose.radar_voxelize(zeroed),
            "torch_pillar_features": lambda: loose.radar_voxel_encoder(tv, tn, tc),
            "torch_scatter": lambda: loose.radar_middle_encoder(tf, tc, n),
            "torch_conv_stack": lambda: loose.radar_bev_conv(tcanvas),
        }, args.reps)

        total = timed({"fused_total": lambda: fused(frames), "torch_total": lambda: loose(frames)}, args.reps)

        # ---- the last layer on the LDS-staged kernel (its input packed from the second layer's fp32 result)
        x2 = loose.radar_bev_conv[1](loose.radar_bev_conv[0](tcanvas)).contiguous()
        ci = ConvImage(n, gy, gx, 64, dev)
        ci.begin([x2]).pack(x2, 0)
        ws, alpha, bias = convs[2][:3]
        staged = ci.conv(ws, alpha, bias)
        one = (ci.amax, 1.0, 0.0)
        direct = RP.conv_bn_relu(convs[2], ci.xs, one, n, gy, gx, out=torch.empty(n, 256, gy, gx, device=dev), staged=False)
        staged_cf = RP.conv_bn_relu(convs[2], ci.xs, one, n, gy, gx, out=torch.empty(n, 256, gy, gx, device=dev), staged=True)
        last = timed({
            "conv_direct_cf_relu": lambda: RP.conv_bn_relu(convs[2], ci.xs, one, n, gy, gx, out=out, staged=False),
            "conv3x3_lds_staged_cf_relu": lambda: RP.conv_bn_relu(convs[2], ci.xs, one, n, gy, gx, out=out, staged=True),
            "conv3x3_lds_staged_channel_last_no_relu": lambda: ci.conv(ws, alpha, bias),
        }, args.reps)
        last["max_abs_diff_direct_vs_staged_channel_last"] = float((torch.relu(staged).permute(0, 3, 1, 2) - direct).abs().max())
        last["max_abs_diff_direct_vs_staged_cf_relu"] = float((staged_cf - direct).abs().max())

    rec = dict(shape=dict(B=B, T=T, points_per_frame=args.points, width=7, grid=[gx, gy, 1], channels=[64, 64, 64, 256],
                          max_num_points=vl.max_num_points, max_voxels=vl.cap()),
               pillars_per_frame=counts, device=torch.cuda.get_device_name(0), unit="ms, median of device-event times", reps=args.reps,
               stages=stages, total=total, last_layer=last, fused_vs_torch_max_abs_diff=agree, output_max_abs=top)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
