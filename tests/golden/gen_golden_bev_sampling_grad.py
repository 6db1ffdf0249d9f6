#!/usr/bin/env python3
"""Golden gradients of BEVSampling: runs the REFERENCE's own module (racformer_transformer.py:429-546 over
bev_self_attention.py, temp_radar=False) on CPU in eval mode (the checkpoint wrapper is bypassed), backpropagates
sum(out * gout) for a seeded gout, and writes a data-only fixture next to this script.  Run in the build container only
(needs the reference tree, see ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_bev_sampling_grad.py

  bev_sampling_grad_small.npz (+ bev_sampling_grad_small.1.npz, .2.npz, ...: the keys dealt over several files, each below the
                        repository's 1 MiB limit for a committed file; a reader merges them)   embed 256, 4 heads, T = 3, NP = 2, D = 5 (P = 10), Q = 21, a 12 x 10 map, d_region = 0.1, for
                        B = 1 (keys "b1:...") and B = 2 ("b2:...", the reference's frame / batch pairing).  Per batch size:
                        query_ray [B,Q,10], query_feat [B,Q,256], bev_feats [B,T,256,12,10], time_diff [B,T], gout, out, and
                        under "g:" the gradients of every parameter, query_feat, bev_feats and query_ray.  The module's
                        weights, shared by both, under their state_dict keys prefixed "w:".  The weights are float16-exact
                        and the BEV maps multiples of 1/8 (stored as float16; the fixture's bulk is the float32 gradients).
Every keypoint is at least 1e-3 of the map away from the clamp bounds 0 / 1 and from the pixel-cell borders, so the float32
and float64 tap choices agree; the queries of the last two rows sit near the rim of the polar grid, where some keypoints fall
clearly outside [0,1] and are clamped.  query_feat is nudged (see nudge) until that holds; asserted below.
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
from racformer_amd import synthetic as syn  # noqa: E402
from racformer_amd.transformer import BEVSampling  # noqa: E402

E, HEADS, T, NP, D, Q, H, W, D_REGION = 256, 4, 3, 2, 5, 21, 12, 10, 0.1
MARGIN = 1e-3


def border_distance(qr, off, ray, td):
    """qr [B,Q,10], off [B,Q,heads*P*2], ray [B,Q,D], td [B,T] (float64) -> [B,Q,heads,P]: the distance of the keypoints of
    point (h, p), over its frames and both coordinates (before the clamp), to the nearest clamp bound or pixel-cell border, in
    map units"""
    from bev_sampling_ref import chain64
    from racformer_amd.transformer import box_table_torch
    res = []
    for b in range(qr.shape[0]):
        loc = chain64(box_table_torch(qr[b:b + 1], syn.PC_RANGE)[0], qr[b, :, 8:10], off[b], ray[b], td[b], HEADS, NP, D,
                      syn.PC_RANGE, D_REGION, clamp=False)                 # [Q,heads,T,P,2]
        ds = []
        for c, n in ((0, W), (1, H)):
            u = loc[..., c]
            cell = u * n - 0.5
            d_cell = (cell - torch.round(cell)).abs() / n
            inside = (u > -0.5 / n) & (u < 1 + 0.5 / n)          # beyond that the clamped coordinate sits on a cell centre
            ds.append(torch.minimum(torch.minimum(u.abs(), (u - 1).abs()), torch.where(inside, d_cell, torch.ones_like(u))))
        res.append(torch.minimum(ds[0], ds[1]).min(2).values)
    return torch.stack(res)


def nudge(mod64, qr, qf, td, rng):
    """query_feat moved a little so that every keypoint keeps 2 * MARGIN: a random search over small changes of the offsets of
    the points that are too close, carried back to query_feat through the pseudo-inverse of the offset / ray Linears (256
    inputs, 85 outputs: an exact solution that leaves the ray logits as they are)"""
    B, Q, _ = qf.shape
    with torch.no_grad():
        off, ray = mod64.sampling_offset(qf), mod64.ray_points_offset(qf)
        delta = torch.zeros(B, Q, HEADS, NP * D, 2, dtype=torch.float64)
        for _ in range(400):
            bad = border_distance(qr, off + delta.reshape(B, Q, -1), ray, td) < 2 * MARGIN
            if not bool(bad.any()):
                break
            trial = delta.clone()
            trial[bad] = torch.from_numpy(rng.uniform(-1.0, 1.0, (int(bad.sum()), 2)))
            ok = border_distance(qr, off + trial.reshape(B, Q, -1), ray, td) >= 2 * MARGIN
            take = bad & ok
            delta[take] = trial[take]
        assert not bool(bad.any()), f"{int(bad.sum())} points could not be moved clear"
        wcat = torch.cat([mod64.sampling_offset.weight, mod64.ray_points_offset.weight])          # [85,256]
        rhs = torch.cat([delta.reshape(B, Q, -1), torch.zeros(B, Q, D, dtype=torch.float64)], dim=-1)
        return qf + rhs @ torch.linalg.pinv(wcat).t()


def main():
    torch.manual_seed(0)
    ref = ref_loader.load_reference()
    rng = np.random.default_rng(71)
    kw = dict(embed_dims=E, num_frames=T, num_points=NP, num_heads=HEADS, num_levels=1, pc_range=list(syn.PC_RANGE),
              spatial_shapes=(W, H), depth_num=D, temp_radar=False)
    rmod = ref.racformer_transformer.BEVSampling(**kw).eval()
    w = {}
    for k, v in rmod.state_dict().items():
        s = 0.5 if "embed" in k else 1.0 / np.sqrt(E)
        w[k] = (rng.standard_normal(tuple(v.shape), dtype=np.float32) * np.float32(s)).astype(np.float16).astype(np.float32)
    w["sampling_offset.bias"] = rng.uniform(-1.5, 1.5, w["sampling_offset.bias"].shape).astype(np.float16).astype(np.float32)
    rmod.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    mod64 = BEVSampling(**kw).eval().double()
    mod64.load_state_dict({k: torch.from_numpy(v).double() for k, v in w.items()})
    d = {"w:" + k: v.astype(np.float16) for k, v in w.items()}
    d["shape"] = np.array([HEADS, T, NP, D, H, W])
    d["d_region"] = np.array(D_REGION)
    for B in (1, 2):
        qr = rng.random((B, Q, 10), dtype=np.float32)
        qr[..., 1] = 0.05 + 0.6 * qr[..., 1]
        qr[:, -2:, 1] = np.float32(0.93)                      # near the rim: keypoints beyond the map, clamped
        qr[:, -2, 0], qr[:, -1, 0] = np.float32(0.02), np.float32(0.27)
        qr[..., 6:8] = qr[..., 6:8] * 2 - 1
        qr[..., 8:10] = qr[..., 8:10] * 4 - 2
        qf = rng.standard_normal((B, Q, E), dtype=np.float32)
        bev = np.round(rng.standard_normal((B, T, E, H, W), dtype=np.float32) * 8) / np.float32(8)
        td = (np.arange(T, dtype=np.float32)[None] * np.float32(0.5) + rng.random((B, T), dtype=np.float32) * np.float32(0.1))
        gout = rng.standard_normal((B, Q, E), dtype=np.float32)
        tqr64, ttd64 = torch.from_numpy(qr).double(), torch.from_numpy(td).double()
        qf = nudge(mod64, tqr64, torch.from_numpy(qf).double(), ttd64, rng).float().numpy()
        with torch.no_grad():
            x = torch.from_numpy(qf).double()
            dmin = float(border_distance(tqr64, mod64.sampling_offset(x), mod64.ray_points_offset(x), ttd64).min())
        assert dmin >= MARGIN, f"B={B}: a keypoint is {dmin:.2e} of the map from a clamp bound or cell border"
        tqf, tqr, tbev = (torch.from_numpy(a).requires_grad_() for a in (qf, qr, bev))
        rmod.zero_grad()
        out = rmod(tqr, tqf, tbev, [dict(time_diff=torch.from_numpy(td))], d_region=D_REGION)
        (out * torch.from_numpy(gout)).sum().backward()
        gq = tqr.grad.numpy()
        assert np.abs(gq[..., [2, 5, 8, 9]]).max() == 0.0 and all(np.abs(gq[..., i]).max() > 0 for i in (0, 1, 3, 4, 6, 7))
        assert bool(out.isfinite().all())
        pre = f"b{B}:"
        d.update({pre + "query_ray": qr, pre + "query_feat": qf, pre + "bev_feats": bev.astype(np.float16), pre + "time_diff": td, pre + "gout": gout,
                  pre + "out": out.detach().numpy(), pre + "g:query_feat": tqf.grad.numpy(), pre + "g:query_ray": gq,
                  pre + "g:bev_feats": tbev.grad.numpy()})
        for k, p in rmod.named_parameters():
            d[pre + "g:" + k] = p.grad.numpy().copy()
        print(f"  B={B}: min distance to a bound / border {dmin:.2e}")
    # deal the keys over files of at most LIMIT raw bytes (largest first; random float data does not compress)
    LIMIT = 960 * 1024
    parts = []
    for k in sorted(d, key=lambda k: -np.asarray(d[k]).nbytes):
        n = np.asarray(d[k]).nbytes
        for part in parts:
            if part[0] + n <= LIMIT:
                part[0] += n
                part[1][k] = d[k]
                break
        else:
            parts.append([n, {k: d[k]}])
    for i, (_, part) in enumerate(parts):
        name = "bev_sampling_grad_small.npz" if i == 0 else f"bev_sampling_grad_small.{i}.npz"
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < 1024 * 1024, name
        print(f"  wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB; {len(part)} keys")


if __name__ == "__main__":
    main()
