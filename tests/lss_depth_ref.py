"""CPU restatement of the depth branch around DepthNet (models/necks/view_transformer_racformer.py:593-699 and
models/necks/focalloss.py:114-125 of the reference) in plain torch, float32 or float64, and -- for the depth-bin edges -- in
numpy float32.  Pinned to the reference by tests/golden/lss_depth_small.npz (tests/test_lss_depth_ref.py); written from the
reference's lines, shares no code with racformer_amd/lss_depth.py.

Maps are [B*N, H, W]; feature pixels [B*N, h, w]; the depth bin D means "no return in range" (background), the RCS class -1
"no class" (where the reference's F.one_hot raises)."""
import os

import numpy as np
import torch


def depth_bin_size(grid_depth):
    lo, hi, n = grid_depth
    return 2 * (hi - lo) / (n * (1 + n))


def blocks(x, ds):
    """[B*N, H, W] -> [B*N*h*w, ds*ds], the reference's view / permute / view"""
    bn, H, W = x.shape
    x = x.view(bn, H // ds, ds, W // ds, ds, 1).permute(0, 1, 3, 5, 2, 4).contiguous()
    return x.view(-1, ds * ds)


def pooled_depth(depth, ds):
    b = blocks(depth, ds)
    b = torch.where(b == 0.0, 1e5 * torch.ones_like(b), b)
    return torch.min(b, dim=-1).values.view(depth.shape[0], depth.shape[1] // ds, depth.shape[2] // ds)


def depth_index(pooled, grid_depth, dtype=torch.float32):
    """the real-valued index -0.5 + 0.5 sqrt(1 + 8 (d - lo) / bin) in ``dtype``; float32: the root taken in float64 and rounded
    once (= the correctly rounded float32 root; torch's own float32 sqrt on the CPU is not)"""
    lo, _, _ = grid_depth
    arg = 1 + 8 * (pooled.to(dtype) - lo) / depth_bin_size(grid_depth)
    return -0.5 + 0.5 * arg.double().sqrt().to(dtype)


def depth_bins(pooled, grid_depth, dtype=torch.float32):
    n = grid_depth[2]
    idx = depth_index(pooled, grid_depth, dtype)
    mask = (idx < 0) | (idx > n) | (~torch.isfinite(idx))
    idx[mask] = n
    return idx.type(torch.int64)


def depth_bins_numpy(d, grid_depth):
    """the yardstick of the bin edges: the plain IEEE float32 sequence in numpy (np.sqrt is correctly rounded)"""
    lo, _, n = grid_depth
    d = np.asarray(d, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = (np.float32(8) * (d - np.float32(lo))) / np.float32(depth_bin_size(grid_depth))
        idx = np.float32(-0.5) + np.float32(0.5) * np.sqrt(np.float32(1) + q)
        bad = (idx < 0) | (idx > n) | ~np.isfinite(idx)
        return np.where(bad, np.float32(n), idx).astype(np.int64)


def edge_depths(grid_depth):
    """d_k = lo + bin k (k + 1) / 2 for k = 0..97 with both float32 neighbours, and the special values"""
    lo = grid_depth[0]
    k = np.arange(98, dtype=np.float64)
    d = (lo + depth_bin_size(grid_depth) * k * (k + 1) / 2).astype(np.float32)
    special = np.asarray([0.0, 0.5, 1e5, np.inf, np.nan, -3.0], np.float32)
    return np.concatenate([d, np.nextafter(d, np.float32(np.inf)), np.nextafter(d, np.float32(-np.inf)), special])


def rcs_class(rcs, ds, grid_rcs):
    """int64 [B*N, h, w] in -1..n-1: the reference's one-hot index minus one, -1 wherever its F.one_hot would raise"""
    lo, hi, n = grid_rcs
    b = blocks(rcs, ds)
    b = torch.where(b < lo, -1e5 * torch.ones_like(b), b)
    m = torch.max(b, dim=-1).values.view(rcs.shape[0], rcs.shape[1] // ds, rcs.shape[2] // ds)
    bin_size = (hi - lo) / n
    r = (m - (lo - bin_size)) / bin_size
    r = torch.where((r < n + 1) & (r >= -1), r, torch.zeros_like(r) - 1)
    return torch.clamp(r.long() - 1, min=-1)


def rcs_one_hot(cls, n):
    return torch.nn.functional.one_hot(cls + 1, num_classes=n + 1)[..., 1:].float()


def prior(bins, cls, weight, bias, D):
    """(rad_dep_grids [B*N, D+1, h, w], rcs_embedding [B*N, E, h, w]) through the dense one-hot tensors, as the reference"""
    dtype = weight.dtype
    ones = torch.ones(bins.shape + (1,), dtype=dtype)
    grids = torch.zeros(bins.shape + (D + 1,), dtype=dtype).scatter_(dim=-1, index=bins.unsqueeze(-1), src=ones).permute(0, 3, 1, 2)
    one_hot = rcs_one_hot(cls, weight.shape[1]).to(dtype).permute(0, 3, 1, 2)
    emb = torch.nn.functional.conv2d(one_hot, weight.view(weight.shape[0], -1, 1, 1), bias)
    return grids, emb


def focal_terms(logits, labels, alpha=0.25, gamma=2.0, eps=1e-6):
    """focalloss.py:114-125, reduction 'none': logits [M, D], labels int64 [M] -> [M]"""
    soft = torch.softmax(logits, dim=1)
    log_soft = torch.log_softmax(logits, dim=1)
    one_hot = torch.zeros_like(logits).scatter_(1, labels.unsqueeze(1), 1.0) + eps
    focal = -alpha * torch.pow(-soft + 1.0, gamma) * log_soft
    return torch.einsum('bc...,bc...->b...', (one_hot, focal))


def depth_loss(preds, bins, weight=3.0, alpha=0.25, gamma=2.0, dtype=torch.float32):
    """(loss, per-pixel terms [B*N, h, w] with zeros at background pixels): get_depth_loss behind the pooling"""
    D = preds.shape[1]
    p = preds.to(dtype).permute(0, 2, 3, 1).contiguous()
    fg = bins < D
    terms = focal_terms(p[fg], bins[fg], alpha, gamma)
    per_pixel = torch.zeros(bins.shape, dtype=dtype).masked_scatter(fg, terms)
    return weight * terms.sum() / max(1.0, fg.sum()), per_pixel


def golden(golden_dir, tag):
    z = np.load(os.path.join(golden_dir, "lss_depth_small.npz"), allow_pickle=False)
    return {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(tag + ":")}


def golden_grid(fx):
    return dict(depth=[float(v) for v in fx["grid_depth"]], rcs=[float(v) for v in fx["grid_rcs"]])


class StandInDepthNet(torch.nn.Module):
    """A two-layer stand-in with DepthNet's forward signature (:546-562): two 1x1 projections (Linear layers over the channel
    axis) of the features concatenated with the two prior tensors, as DepthNet's dep_proj sees them; mlp_input gates the hidden
    layer per camera."""

    def __init__(self, in_channels, prior_channels, mid_channels, out_channels):
        super().__init__()
        self.proj = torch.nn.Linear(in_channels + prior_channels, mid_channels)
        self.mlp = torch.nn.Linear(9, mid_channels)
        self.out = torch.nn.Linear(mid_channels, out_channels)

    def forward(self, x, radar_feats, rcs_embedding, mlp_input):
        y = torch.relu(self.proj(torch.cat((x, radar_feats, rcs_embedding), dim=1).permute(0, 2, 3, 1)))
        gate = torch.sigmoid(self.mlp(mlp_input.reshape(-1, mlp_input.shape[-1])))[:, None, None, :]
        return self.out(y * gate).permute(0, 3, 1, 2)
