#!/usr/bin/env python3
"""Golden vectors of the hard-level sampling path: runs the REFERENCE's own msmv_sampling_v2 (wrapper.py:41-76) and
sampling_4d(aggregate=False) (sparsebev_sampling.py:28-134) on CPU, on seeded inputs, and writes data-only fixtures next to
this script.  Run in the build container only (needs the reference tree, see ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_v2.py

  msmv_v2_small.npz     msmv_sampling_v2 with L = 2, 4 and 5 (prefixes l2_, l4_, l5_): channel-last features, locations
                        (some outside [0,1]), weight rows with exact ties, a NaN and all -inf, the output [S,Q,C,P], and the
                        gradients of sum(out * gout) for the features (channel-last) and the locations
  sampling4d_v2_small.npz
                        sampling_4d(..., aggregate=False): final, homo, i_view, with points visible in no camera
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


def crafted_weights(rng, S, Q, P, L):
    w = rng.random((S, Q, P, L), dtype=np.float32)
    w[0, 0, 0] = 0.3                       # all equal: level 0
    w[0, 0, 1, :] = 0.1
    w[0, 0, 1, L - 1] = 0.7
    w[0, 0, 1, 1] = 0.7                    # tie between 1 and L-1: level 1
    w[0, 0, 2] = -np.inf                   # all -inf: level 0
    w[0, 0, 3, :] = 0.5
    w[0, 0, 3, 1] = np.nan                 # a NaN counts as maximal: level 1
    w[0, 0, 4, :] = 0.1
    w[0, 0, 4, L - 1] = np.nan             # NaN in the last slot beats larger values: level L-1
    w[0, 0, 4, 0] = 0.9
    w[1, 0, 0, :] = 0.2
    w[1, 0, 0, 0] = np.nan
    w[1, 0, 0, L - 1] = np.nan             # two NaNs: the first, level 0
    return w


def gen_msmv_v2(ref):
    wr = ref.wrapper
    rng = np.random.default_rng(31)
    S, N, C, Q, P = 3, 3, 8, 5, 6
    all_hws = [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]
    d = {}
    for L in (2, 4, 5):
        hws = all_hws[:L]
        feats_cl = [rng.standard_normal((S, N, h, w, C), dtype=np.float32) for h, w in hws]
        loc = rng.random((S, Q, P, 3), dtype=np.float32) * 1.1 - 0.05
        loc[..., 2] = rng.integers(0, N, size=(S, Q, P)).astype(np.float32) / np.float32(N - 1)
        loc[2, 1, :, :2] = rng.random((P, 2), dtype=np.float32) * 3.0 - 1.0    # stress: well outside [0,1]
        loc[2, 2, 0, :2] = (0.0, 0.0)
        loc[2, 2, 1, :2] = (1.0, 1.0)
        w = crafted_weights(rng, S, Q, P, L)
        gout = rng.standard_normal((S, Q, C, P), dtype=np.float32)
        feats_cf = [torch.from_numpy(f).permute(0, 4, 1, 2, 3).contiguous().requires_grad_() for f in feats_cl]
        tl = torch.from_numpy(loc).requires_grad_()
        out = wr.msmv_sampling_v2(feats_cf, tl, torch.from_numpy(w))
        (out * torch.from_numpy(gout)).sum().backward()
        k = f"l{L}_"
        d.update({k + "loc": loc, k + "w": w, k + "gout": gout, k + "out": out, k + "gloc": tl.grad})
        d.update({f"{k}feat{i}": f for i, f in enumerate(feats_cl)})
        d.update({f"{k}gfeat{i}": f.grad.permute(0, 2, 3, 4, 1).contiguous() for i, f in enumerate(feats_cf)})
    save("msmv_v2_small.npz", **d)


def gen_sampling4d_v2(ref):
    sp = ref.sparsebev_sampling
    rng = np.random.default_rng(37)
    B, Q, T, G, P, N, L, C = 1, 7, 3, 4, 5, 6, 4, 4
    hws = [(8, 22), (4, 11), (2, 6), (1, 3)]
    H, W = 64, 176
    feats_cl = [rng.standard_normal((B * T * G, N, h, w, C), dtype=np.float32) for h, w in hws]
    feats_cf = [torch.from_numpy(f).permute(0, 4, 1, 2, 3).contiguous() for f in feats_cl]
    pts = rng.standard_normal((B, Q, T, G, P, 3), dtype=np.float32) * np.float32(15.0)
    pts[..., 2] = pts[..., 2] * 0.1 + 1.0
    pts[0, 0, :, :, :2, 2] = 500.0         # far above the rig: visible in no camera
    sw = rng.standard_normal((B, Q, G, T, P, L), dtype=np.float32)
    sw = (np.exp(sw) / np.exp(sw).sum(-1, keepdims=True)).astype(np.float32)
    l2i = np.asarray(syn.ring_lidar2img(T, N, (H, W))).astype(np.float32)[None]
    final, homo, i_view = sp.sampling_4d(torch.from_numpy(pts), feats_cf, torch.from_numpy(sw), torch.from_numpy(l2i), H, W,
                                         aggregate=False)
    d = {f"feat{i}": f for i, f in enumerate(feats_cl)}
    save("sampling4d_v2_small.npz", pts=pts, scale_weights=sw, lidar2img=l2i, image_hw=np.array([H, W]), final=final,
         homo=homo, i_view=i_view, **d)


def main():
    torch.manual_seed(0)
    ref = ref_loader.load_reference()
    gen_msmv_v2(ref)
    gen_sampling4d_v2(ref)


if __name__ == "__main__":
    main()
