#!/usr/bin/env python3
"""Golden gradients of sampling_4d: runs the REFERENCE's own sampling_4d (sparsebev_sampling.py:28-134) on CPU, where its
msmv_sampling / msmv_sampling_v2 take the differentiable grid_sample path (wrapper.py:15-76), backpropagates
sum(final * gout) for a seeded gout, and writes a data-only fixture next to this script.  Run in the build container only
(needs the reference tree, see ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_grad4d.py

  sampling4d_grad_small.npz   two cases, prefixes l4_ (C = 8, L = 4: the generic kernels) and l5_ (C = 64, L = 5: the
                              C = 64 kernels), both with B = 2 and T*G > 1.  Inputs: pts [B,Q,T,G,P,3], scale_weights
                              [B,Q,G,T,P,L], lidar2img [B,T*N,4,4], image_hw, feat{l} channel-last [B*T*G,N,H,W,C], gout
                              [B,Q,G,T*P,C].  Gradients of aggregate=True (agg_) and aggregate=False (hard_): gpts
                              (sample_points), gfeat{l} (channel-last), and gsw (scale_weights, aggregate mode only: argmax
                              cuts the graph in hard-level mode).  Some points are visible in no camera, some lie within a
                              pixel of camera 0's image edges (inside and outside).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_loader  # noqa: E402
from racformer_amd import synthetic as syn  # noqa: E402


def save(name, **arrs):
    path = os.path.join(HERE, name)
    out = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrs.items()}
    np.savez_compressed(path, **out)
    print(f"  wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB")


def rig(B, T, N, H, W):
    """[B, T*N, 4, 4] float32: the ring rig, turned a little for the second batch element"""
    out = []
    for b in range(B):
        c, s = np.cos(0.3 * b), np.sin(0.3 * b)
        ego = np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
        out.append(np.stack([m @ ego for m in syn.ring_lidar2img(T, N, (H, W))]))
    return np.stack(out).astype(np.float32)


def edge_points(l2i_b, H, W):
    """points of camera 0 of frame 0 at normalised (u, v) just inside and just outside its image edges, 12 m deep"""
    uv = [(0.999, 0.5), (1.0004, 0.5), (0.5, 0.0006), (0.5, -0.0007), (0.0005, 0.3), (-0.0006, 0.7), (0.9993, 0.9995),
          (0.25, 0.9996)]
    inv = np.linalg.inv(l2i_b[0].astype(np.float64))
    d = 12.0
    return np.stack([(inv @ np.array([u * W * d, v * H * d, d, 1.0]))[:3] for u, v in uv]).astype(np.float32)


def case(ref, rng, B, Q, T, G, P, N, C, hws):
    sp = ref.sparsebev_sampling
    H, W = 64, 176
    L = len(hws)
    S = B * T * G
    feats_cl = [rng.standard_normal((S, N, h, w, C), dtype=np.float32) for h, w in hws]
    pts = rng.standard_normal((B, Q, T, G, P, 3), dtype=np.float32) * np.float32(15.0)
    pts[..., 2] = pts[..., 2] * 0.1 + 1.0
    pts[0, 0, :, :, :2, 2] = 500.0                     # far above the rig: visible in no camera
    l2i = rig(B, T, N, H, W)
    e = edge_points(l2i[1], H, W)
    flat = pts[1, 1].reshape(T * G * P, 3)             # batch element 1, query 1: the edge points in every (t, g)
    flat[:e.shape[0]] = e
    pts[1, 1] = flat.reshape(T, G, P, 3)
    sw = rng.standard_normal((B, Q, G, T, P, L), dtype=np.float32)
    sw = (np.exp(sw) / np.exp(sw).sum(-1, keepdims=True)).astype(np.float32)
    gout = rng.standard_normal((B, Q, G, T * P, C), dtype=np.float32)
    d = dict(pts=pts, scale_weights=sw, lidar2img=l2i, image_hw=np.array([H, W]), gout=gout)
    d.update({f"feat{i}": f for i, f in enumerate(feats_cl)})
    for mode, aggregate in (("agg_", True), ("hard_", False)):
        feats_cf = [torch.from_numpy(f).permute(0, 4, 1, 2, 3).contiguous().requires_grad_() for f in feats_cl]
        tp = torch.from_numpy(pts).requires_grad_()
        tw = torch.from_numpy(sw).requires_grad_()
        res = sp.sampling_4d(tp, feats_cf, tw, torch.from_numpy(l2i), H, W, aggregate=aggregate)
        final = res if aggregate else res[0]
        assert tuple(final.shape) == gout.shape
        (final * torch.from_numpy(gout)).sum().backward()
        d[mode + "final"] = final
        d[mode + "gpts"] = tp.grad
        if aggregate:
            d[mode + "gsw"] = tw.grad
        else:
            assert tw.grad is None or float(tw.grad.abs().max()) == 0.0
        d.update({f"{mode}gfeat{i}": f.grad.permute(0, 2, 3, 4, 1).contiguous() for i, f in enumerate(feats_cf)})
    return d


def main():
    torch.manual_seed(0)
    ref = ref_loader.load_reference()
    rng = np.random.default_rng(41)
    d = {}
    for k, v in case(ref, rng, B=2, Q=5, T=2, G=2, P=5, N=3, C=8, hws=[(6, 16), (3, 8), (2, 4), (1, 2)]).items():
        d["l4_" + k] = v
    for k, v in case(ref, rng, B=2, Q=4, T=2, G=1, P=6, N=3, C=64, hws=[(4, 8), (2, 4), (2, 2), (1, 2), (1, 1)]).items():
        d["l5_" + k] = v
    save("sampling4d_grad_small.npz", **d)


if __name__ == "__main__":
    main()
