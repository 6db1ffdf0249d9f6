#!/usr/bin/env python3
"""Golden gradients of RaCFormerSampling: runs the REFERENCE's own module (racformer_transformer.py:338-427, inner_forward:
the checkpoint wrapper is bypassed) on CPU, where its msmv_sampling takes the differentiable grid_sample path
(wrapper.py:15-76), backpropagates sum(out * gout) for a seeded gout, and writes a data-only fixture next to this script.
Run in the build container only (needs the reference tree, see ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_racsampling_grad.py

  racsampling_grad_small.npz   embed 256, G = 4, T = 2, NP = 2, D = 3 (P = 6), Q = 21, a 2-camera rig (front and back: most of
                        the circle unseen, so many points have no valid camera and are sampled in camera 0, some of them behind
                        it with homo <= eps), 4 levels (4x12, 2x6, 1x3, 1x2), image 64 x 176, d_region = 0.1, B = 1.
                        query_ray [1,Q,10], query_feat [1,Q,256], feat{l} channel-last [S,N,H,W,64] (multiples of 1/8, stored
                        as float16), time_diff [1,T], lidar2img [1,T*N,4,4], gout, out, and under "g:" the gradients of every
                        parameter, query_feat, query_ray and feat{l}.  The module's weights under their state_dict keys
                        prefixed "w:" (float16-exact).  The queries of the last two rows sit near the rim of the polar grid,
                        where keypoints fall outside [0,1] and are clamped.
The chain is evaluated in float32 and in float64 (tests/sampling4d_core_ref.py); the seed is advanced until both make the same
camera choice, the same clamp gates, the same homo > eps gate and the same floor in every level for EVERY keypoint (asserted
below; the seed is stored), so no test has to set keypoints aside.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import ref_loader  # noqa: E402
import sampling4d_core_ref as SR  # noqa: E402
from racformer_amd import synthetic as syn  # noqa: E402
from racformer_amd.transformer import box_table_torch  # noqa: E402

E, G, T, NP, D, Q, N, D_REGION = 256, 4, 2, 2, 3, 21, 2, 0.1
IMG_HW = (64, 176)
HWS = [(4, 12), (2, 6), (1, 3), (1, 2)]
L = len(HWS)
RANGE = (0.15, 0.65)     # of the queries' polar distance (x 65 m)
FIRST_SEED = 91


def discrete_steps(w, qr, qf, td, l2i, dtype):
    """camera choice, clamp gates, homo gate and the tap cell of every level, for every keypoint, with the chain in ``dtype``"""
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)  # noqa: E731
    x = t(qf)
    lin = {k: x @ t(w[k + ".weight"]).t() + t(w[k + ".bias"]) for k in ("sampling_offset", "ray_points_offset")}
    qb = t(qr)
    c = SR.chain64(box_table_torch(qb, syn.PC_RANGE), qb[..., 8:10], lin["sampling_offset"], lin["ray_points_offset"], t(td), t(l2i),
                   G, NP, D, syn.PC_RANGE, D_REGION, IMG_HW[0], IMG_HW[1])
    gates = torch.stack([(c["ux"] >= 0) & (c["ux"] <= 1), (c["uy"] >= 0) & (c["uy"] <= 1), c["homo"] > 1e-5, c["any_valid"]], -1)
    return c["view"], gates, SR.floors(c["u"], c["v"], HWS)


def draw(seed):
    rng = np.random.default_rng(seed)
    qr = rng.random((1, Q, 10), dtype=np.float32)
    qr[..., 1] = RANGE[0] + (RANGE[1] - RANGE[0]) * qr[..., 1]     # no keypoint within arm's reach of a camera
    qr[:, -2:, 1] = np.float32(0.93)                      # near the rim: keypoints beyond the map, clamped
    qr[:, -2, 0], qr[:, -1, 0] = np.float32(0.02), np.float32(0.27)
    qr[..., 6:8] = qr[..., 6:8] * 2 - 1
    qr[..., 8:10] = qr[..., 8:10] * 4 - 2
    qf = rng.standard_normal((1, Q, E), dtype=np.float32)
    feats = [np.round(rng.standard_normal((T * G, N, h, w, 64), dtype=np.float32) * 8) / np.float32(8) for h, w in HWS]
    td = (np.arange(T, dtype=np.float32)[None] * np.float32(0.5) + rng.random((1, T), dtype=np.float32) * np.float32(0.1))
    gout = rng.standard_normal((1, Q, G, T * NP * D, 64), dtype=np.float32)
    l2i = np.stack(syn.ring_lidar2img(T, N, IMG_HW))[None].astype(np.float32)
    return qr, qf, feats, td, gout, l2i


def main():
    torch.manual_seed(0)
    ref = ref_loader.load_reference()
    kw = dict(embed_dims=E, num_frames=T, num_groups=G, num_points=NP, num_levels=L, depth_num=D, pc_range=list(syn.PC_RANGE))
    rmod = ref.racformer_transformer.RaCFormerSampling(**kw).eval()
    wrng = np.random.default_rng(83)
    w = {}
    for k, v in rmod.state_dict().items():
        w[k] = (wrng.standard_normal(tuple(v.shape), dtype=np.float32) * np.float32(1.0 / np.sqrt(E))).astype(np.float16).astype(np.float32)
    w["sampling_offset.bias"] = wrng.uniform(-1.5, 1.5, w["sampling_offset.bias"].shape).astype(np.float16).astype(np.float32)
    rmod.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    seed = FIRST_SEED
    while True:
        qr, qf, feats, td, gout, l2i = draw(seed)
        v32, g32, f32 = discrete_steps(w, qr, qf, td, l2i, torch.float32)
        v64, g64, f64 = discrete_steps(w, qr, qf, td, l2i, torch.float64)
        if torch.equal(v32, v64) and torch.equal(g32, g64) and torch.equal(f32, f64):
            break
        print(f"  seed {seed}: float32 and float64 differ in a discrete step; next")
        seed += 1
    assert torch.equal(v32, v64) and torch.equal(g32, g64) and torch.equal(f32, f64)
    n_kp = g64[..., 0].numel()
    print(f"  seed {seed}: {n_kp} keypoints; clamped x/y {int((~g64[..., 0]).sum())}/{int((~g64[..., 1]).sum())}, "
          f"homo <= eps {int((~g64[..., 2]).sum())}, no valid camera {int((~g64[..., 3]).sum())}")
    assert int((~g64[..., 0]).sum()) > 0 and int((~g64[..., 2]).sum()) > 0 and int((~g64[..., 3]).sum()) > 0
    tqr, tqf = torch.from_numpy(qr).requires_grad_(), torch.from_numpy(qf).requires_grad_()
    tfe = [torch.from_numpy(f).permute(0, 4, 1, 2, 3).contiguous().requires_grad_() for f in feats]       # [S,C,N,H,W]
    metas = [dict(img_shape=[(IMG_HW[0], IMG_HW[1], 3)], time_diff=torch.from_numpy(td), lidar2img=torch.from_numpy(l2i))]
    out = rmod.inner_forward(tqr, tqf, tfe, metas, d_region=D_REGION)
    assert tuple(out.shape) == gout.shape and bool(out.isfinite().all())
    (out * torch.from_numpy(gout)).sum().backward()
    gq = tqr.grad.numpy()
    assert np.abs(gq[..., [8, 9]]).max() == 0.0 and all(np.abs(gq[..., i]).max() > 0 for i in range(8))
    d = {"w:" + k: v.astype(np.float16) for k, v in w.items()}
    d.update(shape=np.array([G, T, NP, D, N, L]), d_region=np.array(D_REGION), image_hw=np.array(IMG_HW), seed=np.array(seed),
             query_ray=qr, query_feat=qf, time_diff=td, lidar2img=l2i, gout=gout, out=out.detach().numpy())
    d.update({f"feat{i}": f.astype(np.float16) for i, f in enumerate(feats)})
    d.update({"g:query_feat": tqf.grad.numpy(), "g:query_ray": gq})
    d.update({f"g:feat{i}": f.grad.permute(0, 2, 3, 4, 1).contiguous().numpy() for i, f in enumerate(tfe)})
    for k, p in rmod.named_parameters():
        d["g:" + k] = p.grad.numpy().copy()
    path = os.path.join(HERE, "racsampling_grad_small.npz")
    np.savez_compressed(path, **d)
    assert os.path.getsize(path) < 1024 * 1024
    print(f"  wrote racsampling_grad_small.npz: {os.path.getsize(path) / 1024:.1f} KiB; {len(d)} keys")


if __name__ == "__main__":
    main()
