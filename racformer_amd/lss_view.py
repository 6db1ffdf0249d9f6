"""Drop-in for the view-transform half of ``LSSViewTransformer_racformer`` (models/necks/view_transformer_racformer.py of
the reference): depth logits, context features and the cameras' ``lidar2img`` in, the channel-first BEV map out, on the HIP
kernels of ``csrc/lss_view.hip`` (``rac_lss_*``).  Differentiable, nothing is read back to the host, and every launch is sized
by an upper bound, so forward and backward can be captured into a graph.

Layouts.  ``depth_digit`` [B*N, D, H, W] and ``tran_feat`` [B*N, C, H, W] are the reference's channel-first tensors; the
features are transposed once to channel-last rows [B*N*H*W, C] (``rac_lss_transpose_fwd``), which is what the gathers read.
The output is [B, Z*C, Y, X] with channel index z*C + c, the order of ``voxel_pooling_v2``'s
``torch.cat(bev_feat.unbind(dim=2), 1)``.  Points of one cell are summed in ascending ``ranks_depth`` (the reference's
``argsort`` leaves that order unspecified); two runs give the same bits.

Out of scope here: DepthNet / ASPP / SE layers.  The radar depth and RCS inputs, the depth loss and the subclass
``LSSViewTransformerBEVDepth_racformer`` are in ``racformer_amd/lss_depth.py``.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib

LSS_CHUNK = 64          # points per splat chunk (csrc/lss_view.hip): sizes the partial-row scratch

Grid = namedtuple("Grid", "lower interval size")                    # (x, y, z) each; size in cells, ints
FrustumTables = namedtuple("FrustumTables", "depth v u")            # float32 [D], [H], [W]
RankTables = namedtuple("RankTables", "cells ranks_bev ranks_depth ranks_feat interval_starts interval_lengths counts")


def make_grid(x, y, z):
    """``Grid`` from the reference's per-axis (lower, upper, interval) configuration, through the same float32 tensors as
    ``create_grid_infos`` (:82-85)."""
    lower = torch.Tensor([cfg[0] for cfg in (x, y, z)])
    interval = torch.Tensor([cfg[2] for cfg in (x, y, z)])
    size = torch.Tensor([(cfg[1] - cfg[0]) / cfg[2] for cfg in (x, y, z)])
    return Grid(tuple(float(v) for v in lower), tuple(float(v) for v in interval), tuple(int(v) for v in size))


def frustum_tables(frustum):
    """The three axes of a [D, H, W, 3] frustum (u, v, d in the last dimension) as contiguous float32 tables."""
    return FrustumTables(frustum[:, 0, 0, 2].contiguous().float(), frustum[0, :, 0, 1].contiguous().float(),
                         frustum[0, 0, :, 0].contiguous().float())


def img2lidar_from_metas(img_metas):
    """[B*N, 4, 4] float32 CPU tensor: ``np.linalg.inv`` of every ``lidar2img`` in the matrices' own dtype, then cast to
    float32 (:139-147).  The matrices arrive as host arrays, so this is an upload, not a read-back."""
    inv = np.asarray([[np.linalg.inv(m) for m in meta["lidar2img"]] for meta in img_metas]).astype(np.float32)
    return torch.from_numpy(inv.reshape(-1, 4, 4))


def _dims(depth_shape, img2lidar, grid, batch):
    bn, d, h, w = depth_shape
    if img2lidar.shape != (bn, 4, 4) or bn % batch != 0:
        raise ValueError(f"lss_view: img2lidar {tuple(img2lidar.shape)} / batch {batch} do not fit {bn} camera images")
    return bn, bn // batch, d, h, w


def lss_cells(img2lidar, tables, grid, batch, depth_shape):
    """int32 [B*N*D*H*W]: every frustum point's BEV cell ``((b*Z + z)*Y + y)*X + x``, or -1 if it falls outside the grid."""
    bn, n, d, h, w = _dims(depth_shape, img2lidar, grid, batch)
    _lib.require_gpu(img2lidar, *tables, what="lss_cells")
    if img2lidar.dtype != torch.float32 or tuple(t.numel() for t in tables) != (d, h, w):
        raise ValueError("lss_cells: float32 matrices and frustum tables of D, H, W entries expected")
    cells = torch.empty(bn * d * h * w, dtype=torch.int32, device=img2lidar.device)
    (lx, ly, lz), (ix, iy, iz), (X, Y, Z) = grid
    rc = _lib.lib().rac_lss_cells_fwd(_lib.ptr(img2lidar), _lib.ptr(tables.depth), _lib.ptr(tables.v), _lib.ptr(tables.u),
                                      _lib.ptr(cells), bn, n, d, h, w, lx, ly, lz, ix, iy, iz, X, Y, Z, _lib.stream_ptr())
    _lib.check(rc, "rac_lss_cells_fwd")
    return cells


def lss_rank_tables(img2lidar, tables, grid, batch, depth_shape, trim=False):
    """``RankTables``: the cell table plus ``ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths`` (int32, the
    dtypes ``racformer_amd.bev_pool.bev_pool_v2`` takes) and the device ``counts`` = (kept points, occupied cells).

    Untrimmed, the rank tables have B*N*D*H*W entries and the interval tables min(cells, points); entries past the counts
    are padding: -1 in the rank tables, start 0 / length 0 in the interval tables.  ``trim=True`` reads the counts back
    once and slices the five tables to them -- what ``bev_pool_v2`` needs (the reference's ``accelerate=True`` path)."""
    bn, n, d, h, w = _dims(depth_shape, img2lidar, grid, batch)
    cells = lss_cells(img2lidar, tables, grid, batch, depth_shape)
    dev = cells.device
    n_points, n_cells = cells.numel(), batch * grid.size[0] * grid.size[1] * grid.size[2]
    n_int = min(n_points, n_cells)
    rb, rd, rf = (torch.empty(n_points, dtype=torch.int32, device=dev) for _ in range(3))
    starts, lengths = (torch.empty(n_int, dtype=torch.int32, device=dev) for _ in range(2))
    counts = torch.empty(2, dtype=torch.int32, device=dev)
    work = torch.empty(3 * n_cells + n_points, dtype=torch.int32, device=dev)
    rc = _lib.lib().rac_lss_tables_fwd(_lib.ptr(cells), _lib.ptr(rb), _lib.ptr(rd), _lib.ptr(rf), _lib.ptr(starts),
                                       _lib.ptr(lengths), _lib.ptr(counts), _lib.ptr(work), n_points, n_cells, d, h * w,
                                       _lib.stream_ptr())
    _lib.check(rc, "rac_lss_tables_fwd")
    if trim:
        n_kept, n_occ = (int(v) for v in counts.cpu())
        rb, rd, rf, starts, lengths = rb[:n_kept], rd[:n_kept], rf[:n_kept], starts[:n_occ], lengths[:n_occ]
    return RankTables(cells, rb, rd, rf, starts, lengths, counts)


def _transpose(src, batch, rows, cols):
    dst = torch.empty(batch * rows * cols, dtype=torch.float32, device=src.device)
    rc = _lib.lib().rac_lss_transpose_fwd(_lib.ptr(src), _lib.ptr(dst), batch, rows, cols, _lib.stream_ptr())
    _lib.check(rc, "rac_lss_transpose_fwd")
    return dst


def lss_view_forward(depth_digit, tran_feat, ranks, grid, batch):
    """The forward launches alone (no autograd): -> (bev [B, Z*C, Y, X], stats [B*N*H*W, 2], feat_cl [B*N*H*W*C]); the last two are
    what ``lss_view_backward`` needs beside the logits and the cell table."""
    _lib.require_gpu(depth_digit, tran_feat, *ranks, what="lss_view_transform")
    if depth_digit.dtype != torch.float32 or tran_feat.dtype != torch.float32:
        raise TypeError("lss_view_transform: float32 logits and features expected")
    bn, d, h, w = depth_digit.shape
    c = tran_feat.shape[1]
    X, Y, Z = grid.size
    n_points, n_cells = bn * d * h * w, batch * X * Y * Z
    if tran_feat.shape != (bn, c, h, w) or ranks.cells.numel() != n_points or ranks.ranks_bev.numel() != n_points \
            or ranks.interval_starts.numel() != min(n_points, n_cells):
        raise ValueError("lss_view_transform: shapes of logits, features and (untrimmed) rank tables do not fit")
    L, dev, st = _lib.lib(), depth_digit.device, _lib.stream_ptr()
    stats = torch.empty(bn * h * w, 2, dtype=torch.float32, device=dev)
    _lib.check(L.rac_lss_softmax_stats_fwd(_lib.ptr(depth_digit), _lib.ptr(stats), bn, d, h * w, st),
               "rac_lss_softmax_stats_fwd")
    feat_cl = _transpose(tran_feat, bn, c, h * w)
    cell_interval = torch.empty(n_cells, dtype=torch.int32, device=dev)
    partial = torch.empty((-(-n_points // LSS_CHUNK) + min(n_points, n_cells)) * c, dtype=torch.float32, device=dev)
    out = torch.empty(batch, Z * c, Y, X, dtype=torch.float32, device=dev)
    rc = L.rac_lss_splat_fwd(_lib.ptr(depth_digit), _lib.ptr(stats), _lib.ptr(feat_cl), _lib.ptr(ranks.ranks_depth),
                             _lib.ptr(ranks.ranks_feat), _lib.ptr(ranks.ranks_bev), _lib.ptr(ranks.interval_starts),
                             _lib.ptr(ranks.interval_lengths), _lib.ptr(ranks.counts), _lib.ptr(cell_interval),
                             _lib.ptr(partial), _lib.ptr(out), n_points, batch, c, X, Y, Z, st)
    _lib.check(rc, "rac_lss_splat_fwd")
    return out, stats, feat_cl


def lss_view_backward(grad_out, depth_digit, stats, feat_cl, cells, grid, batch):
    """The backward launches alone: grad_out [B, Z*C, Y, X] -> (grad_logits [B*N,D,H,W], grad_feat [B*N,C,H,W])."""
    bn, d, h, w = depth_digit.shape
    X, Y, Z = grid.size
    c = grad_out.shape[1] // Z
    grad_out = grad_out.contiguous().float()
    _lib.require_gpu(grad_out, depth_digit, stats, feat_cl, cells, what="lss_view_backward")
    grad_cell = _transpose(grad_out, batch * Z, c, Y * X)                  # [B*Z*Y*X, C]
    grad_feat_cl = torch.empty(bn * h * w * c, dtype=torch.float32, device=grad_out.device)
    grad_logits = torch.empty_like(depth_digit)
    rc = _lib.lib().rac_lss_view_bwd(_lib.ptr(grad_cell), _lib.ptr(depth_digit), _lib.ptr(stats), _lib.ptr(feat_cl),
                                     _lib.ptr(cells), _lib.ptr(grad_feat_cl), _lib.ptr(grad_logits), bn, c, d, h * w,
                                     _lib.stream_ptr())
    _lib.check(rc, "rac_lss_view_bwd")
    return grad_logits, _transpose(grad_feat_cl, bn, h * w, c).view(bn, c, h, w)


class LSSViewFunction(torch.autograd.Function):
    """(depth_digit [B*N,D,H,W], tran_feat [B*N,C,H,W], untrimmed RankTables, Grid, B) -> bev [B, Z*C, Y, X]."""

    @staticmethod
    def forward(ctx, depth_digit, tran_feat, ranks, grid, batch):
        out, stats, feat_cl = lss_view_forward(depth_digit, tran_feat, ranks, grid, batch)
        ctx.save_for_backward(depth_digit, stats, feat_cl, ranks.cells)
        ctx.grid, ctx.batch = grid, batch
        return out

    @staticmethod
    def backward(ctx, grad_out):
        depth_digit, stats, feat_cl, cells = ctx.saved_tensors
        return lss_view_backward(grad_out, depth_digit, stats, feat_cl, cells, ctx.grid, ctx.batch) + (None, None, None)


def lss_view_transform(depth_digit, tran_feat, img2lidar, tables, grid, batch, ranks=None):
    """The Lift-Splat view transform: softmax over the D logits, lift, splat.  -> bev [B, Z*C, Y, X].

    ``img2lidar`` [B*N,4,4] float32 on the device, ``tables`` a ``FrustumTables``, ``grid`` a ``Grid``.  ``ranks``: untrimmed
    ``RankTables`` of an earlier ``lss_rank_tables`` call to reuse (``accelerate=True``); built here when None."""
    _lib.require_gpu(depth_digit, tran_feat, what="lss_view_transform")
    if ranks is None:
        ranks = lss_rank_tables(img2lidar, tables, grid, batch, tuple(depth_digit.shape))
    return LSSViewFunction.apply(depth_digit, tran_feat, ranks, grid, batch)


class LSSViewTransformer_racformer(nn.Module):
    """The reference's module with its constructor arguments and state-dict keys (``frustum``, ``depth_net.weight``,
    ``depth_net.bias``); ``view_transform_core`` runs on the HIP kernels.  ``accelerate=True`` keeps the rank tables of the
    first call (the reference's ``pre_compute``): later calls ignore their matrices.  The 1x1 ``depth_net`` stays a torch
    convolution (outside this operator)."""

    def __init__(self, grid_config, input_size, downsample=16, in_channels=512, out_channels=64, accelerate=False,
                 norm_cfg=dict(type='BN'), depth_only=False):
        super().__init__()
        self.grid_config = grid_config
        self.downsample = downsample
        lo, hi, n = grid_config['depth']
        # quadratically spaced depth bins (:52-54)
        self.bin_size = 2 * (hi - lo) / (n * (1 + n))
        bin_indice = torch.linspace(0, n - 1, int(n), requires_grad=False)
        self.bin_value = (bin_indice + 0.5).pow(2) * self.bin_size / 2 - self.bin_size / 8 + lo
        self.create_grid_infos(**grid_config)
        self.create_frustum(input_size, downsample)
        self.out_channels = out_channels
        self.in_channels = in_channels
        self.depth_net = nn.Conv2d(in_channels, self.D if depth_only else self.D + out_channels, kernel_size=1, padding=0)
        self.accelerate = accelerate
        self.initial_flag = True
        self.ranks = None

    def create_grid_infos(self, x, y, z, **kwargs):
        self.grid_lower_bound = torch.Tensor([cfg[0] for cfg in [x, y, z]])
        self.grid_interval = torch.Tensor([cfg[2] for cfg in [x, y, z]])
        self.grid_size = torch.Tensor([(cfg[1] - cfg[0]) / cfg[2] for cfg in [x, y, z]])
        self.grid = make_grid(x, y, z)

    def create_frustum(self, input_size, downsample):
        """u = linspace(0, W_in-1, W_feat), v = linspace(0, H_in-1, H_feat), d = bin_value, as float32 tensors; the [D,H,W,3]
        ``frustum`` parameter is the reference's, the three axis tables (non-persistent buffers) are what the kernel reads."""
        H_in, W_in = input_size
        H_feat, W_feat = H_in // downsample, W_in // downsample
        self.D = self.bin_value.shape[0]
        d = self.bin_value.view(-1, 1, 1).expand(-1, H_feat, W_feat)
        x = torch.linspace(0, W_in - 1, W_feat, dtype=torch.float).view(1, 1, W_feat).expand(self.D, H_feat, W_feat)
        y = torch.linspace(0, H_in - 1, H_feat, dtype=torch.float).view(1, H_feat, 1).expand(self.D, H_feat, W_feat)
        self.frustum = nn.Parameter(torch.stack((x, y, d), -1), requires_grad=False)
        t = frustum_tables(self.frustum.data)
        self.register_buffer("depth_table", t.depth.clone(), persistent=False)
        self.register_buffer("v_table", t.v.clone(), persistent=False)
        self.register_buffer("u_table", t.u.clone(), persistent=False)

    def _rank_tables(self, depth_digit, img_metas):
        m = img2lidar_from_metas(img_metas).to(depth_digit.device)
        t = FrustumTables(self.depth_table, self.v_table, self.u_table)
        return lss_rank_tables(m, t, self.grid, len(img_metas), tuple(depth_digit.shape))

    def pre_compute(self, depth_digit, img_metas):
        if self.initial_flag:
            self.ranks = self._rank_tables(depth_digit, img_metas)
            self.initial_flag = False

    def view_transform_core(self, x, depth_digit, tran_feat, img_metas):
        depth_digit = depth_digit.contiguous()
        _lib.require_gpu(depth_digit, what="LSSViewTransformer_racformer")
        ranks = self.ranks if self.accelerate else self._rank_tables(depth_digit, img_metas)
        bev_feat = LSSViewFunction.apply(depth_digit, tran_feat.contiguous(), ranks, self.grid, len(img_metas))
        return bev_feat, depth_digit

    def view_transform(self, x, depth_digit, tran_feat, img_metas):
        if self.accelerate:
            depth_digit = depth_digit.contiguous()
            _lib.require_gpu(depth_digit, what="LSSViewTransformer_racformer")
            self.pre_compute(depth_digit, img_metas)
        return self.view_transform_core(x, depth_digit, tran_feat, img_metas)

    def forward(self, x, img_metas):
        """x [B, N, C_in, H, W] -> (bev_feat [B, Z*C, Y, X], depth_digit [B*N, D, H, W])."""
        B, N, C, H, W = x.shape
        x = F.conv2d(x.view(B * N, C, H, W), self.depth_net.weight, self.depth_net.bias)
        depth_digit = x[:, :self.D, ...]
        tran_feat = x[:, self.D:self.D + self.out_channels, ...]
        return self.view_transform(x, depth_digit, tran_feat, img_metas)

    def get_mlp_input(self, rot, tran, intrin, post_rot, post_tran, bda):
        return None
