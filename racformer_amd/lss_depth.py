"""The depth branch around ``DepthNet`` of ``LSSViewTransformerBEVDepth_racformer`` (models/necks/view_transformer_racformer.py
:572-699 and models/necks/focalloss.py of the reference) on the HIP kernels of ``csrc/lss_depth.hip``: the radar depth and RCS
maps pooled to the feature resolution and binned in one pass, the prior tensor ``DepthNet`` concatenates behind its features
(one-hot radar depth grid + ``rcs_embedding`` of the RCS class, without the one-hot input), and ``loss_depth``.  Differentiable,
nothing is read back to the host, every launch is sized by shapes: forward and backward can be captured into a graph and two runs
give the same bits.

Three layers:
  functional   ``pool_bins``, ``radar_prior``, ``depth_loss`` -- the kernels on device tensors, the torch restatement on CPU tensors
  restatement  ``pool_bins_torch``, ``radar_prior_torch``, ``softmax_focal_loss``, ``depth_loss_torch`` -- the reference's tensor
               operations on any device in the inputs' dtype (the CPU route, and what the kernels are compared and timed against)
  module       ``LSSViewTransformerBEVDepth_racformer`` with the reference's constructor arguments, method signatures and
               state-dict keys; ``depth_net`` is passed in (any module with DepthNet's forward), or built by ``from_config`` as
               this package's ``depth_net.DepthNet`` -- on its HIP route the prior tensor is never built

Index maps are int32 [B*N, h, w]: the depth bin in 0..D (D = no radar return in range: the background label of the loss and
the last channel of the one-hot grid) and the RCS class in -1..n_rcs-1.  Class -1 is "no class" -- an all-below-range block, a
block maximum >= the upper bound, or NaN: an all-zero one-hot row, ``bias`` alone in the embedding.  The reference's
``F.one_hot`` raises on these inputs; everywhere else the two agree.

The depth bin follows the reference's float32 operations with IEEE division and a correctly rounded square root (torch's CPU
``sqrt`` is not: the restatement takes the root in float64 and rounds once, which is the correctly rounded float32 root).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .depth_net import DepthNet
from .lss_view import LSSViewTransformer_racformer, RankTables, img2lidar_from_metas

EMPTY_DEPTH, EMPTY_RCS = 1e5, -1e5
ONE_HOT_EPS = 1e-6
PRIOR_BWD_SEGMENTS = 8  # pixel segments of rac_lss_prior_bwd (csrc/lss_depth.hip): sizes its scratch


def bin_constants(grid_config):
    """(depth_lo, depth_bin_size, D), (rcs_lo, rcs_lo - rcs_bin, rcs_bin, n_rcs) as Python floats / ints, computed in double
    as the reference does (:614, :656); the rcs tuple is None without an ``rcs`` entry."""
    lo, hi, n = grid_config["depth"]
    depth = (float(lo), 2 * (hi - lo) / (n * (1 + n)), int(n))
    rcs = None
    if "rcs" in grid_config:
        rlo, rhi, rn = grid_config["rcs"]
        rbin = (rhi - rlo) / rn
        rcs = (float(rlo), rlo - rbin, rbin, int(rn))
    return depth, rcs


def _block_view(x, ds):
    bn, H, W = x.shape
    if ds < 1 or H % ds or W % ds:
        raise ValueError(f"lss_depth: a {H} x {W} map is not a multiple of downsample={ds}")
    return x.view(bn, H // ds, ds, W // ds, ds).permute(0, 1, 3, 2, 4).reshape(bn, H // ds, W // ds, ds * ds)


def _sqrt(x):
    return x.double().sqrt().to(x.dtype) if x.dtype == torch.float32 else x.sqrt()


# ------------------------------------------------------------------------------------------------------------ restatement
def pool_bins_torch(depth, rcs, grid_config, downsample):
    """get_downsampled_depth (:593-630) and the class of get_downsampled_rcs (:633-662) in torch, in the maps' dtype.
    depth, rcs: [B*N, H, W] or None -> (pooled [B*N,h,w], bins int32, rcs_class int32), None where the map is None."""
    (dlo, dbin, dn), rc = bin_constants(grid_config)
    pooled = bins = cls = None
    if depth is not None:
        blocks = _block_view(depth, downsample)
        pooled = torch.where(blocks == 0.0, EMPTY_DEPTH * torch.ones_like(blocks), blocks).min(dim=-1).values
        idx = -0.5 + 0.5 * _sqrt(1 + 8 * (pooled - dlo) / dbin)
        bad = (idx < 0) | (idx > dn) | (~torch.isfinite(idx))
        bins = torch.where(bad, torch.full_like(idx, dn), idx).to(torch.int32)
    if rcs is not None:
        rlo, roff, rbin, rn = rc
        blocks = _block_view(rcs, downsample)
        m = torch.where(blocks < rlo, EMPTY_RCS * torch.ones_like(blocks), blocks).max(dim=-1).values
        r = (m - roff) / rbin
        r = torch.where((r < rn + 1) & (r >= -1), r, torch.zeros_like(r) - 1)
        cls = (r.to(torch.int32) - 1).clamp(min=-1)
    return pooled, bins, cls


def radar_prior_torch(bins, rcs_class, weight, bias, D):
    """[B*N, (D+1)+E, h, w]: one-hot of ``bins`` over D+1 channels (rad_dep_grids, :690-693) | weight[:, class] + bias
    (rcs_embedding of the one-hot RCS map, :688), bias alone for class -1.  weight [E, n_rcs(, 1, 1)]."""
    w2 = weight.reshape(weight.shape[0], -1)
    grid = (bins.unsqueeze(1) == torch.arange(D + 1, device=bins.device).view(1, -1, 1, 1)).to(w2.dtype)
    cls = rcs_class.long()
    emb = w2[:, cls.clamp(min=0)].permute(1, 0, 2, 3)
    emb = torch.where((cls >= 0).unsqueeze(1), emb, torch.zeros_like(emb)) + bias.view(1, -1, 1, 1)
    return torch.cat((grid, emb), 1)


def softmax_focal_loss(input, target, alpha, gamma=2.0, eps=ONE_HOT_EPS):
    """focalloss.py:114-125 with reduction 'none': input [N, C, *] logits, target [N, *] int64 -> [N, *]."""
    input_soft = F.softmax(input, dim=1)
    log_input_soft = F.log_softmax(input, dim=1)
    one_hot = torch.zeros_like(input).scatter_(1, target.unsqueeze(1), 1.0) + eps
    weight = torch.pow(-input_soft + 1.0, gamma)
    focal = -alpha * weight * log_input_soft
    return (one_hot * focal).sum(1)


def depth_loss_torch(depth_preds, bins, alpha=0.25, gamma=2.0, weight=3.0):
    """get_depth_loss (:666-678) behind the pooling, the reference's steps: the boolean-mask gather of the foreground pixels
    (label < D) and ``max(1.0, count)`` on a tensor -- two host syncs on a device."""
    D = depth_preds.shape[1]
    preds = depth_preds.permute(0, 2, 3, 1).contiguous()
    fg = bins < D
    labels = bins[fg].long()
    loss = softmax_focal_loss(preds[fg], labels, alpha, gamma)
    return weight * loss.sum() / max(1.0, fg.sum())


# ------------------------------------------------------------------------------------------------------------ kernels
def _on_device(*tensors):
    return any(t is not None and t.is_cuda for t in tensors)


def pool_bins(depth, rcs, grid_config, downsample):
    """depth, rcs: float32 [B*N, H, W] maps (either may be None) -> (pooled depth f32, depth bins int32, rcs class int32), each
    [B*N, h, w] or None; one launch (``rac_lss_pool_bins_fwd``) on device tensors, ``pool_bins_torch`` on CPU tensors."""
    if depth is None and rcs is None:
        raise ValueError("pool_bins: neither a depth nor an RCS map")
    if not _on_device(depth, rcs):
        return pool_bins_torch(depth, rcs, grid_config, downsample)
    some = depth if depth is not None else rcs
    maps = [t for t in (depth, rcs) if t is not None]
    _lib.require_gpu(*maps, what="pool_bins")
    if any(t.dtype != torch.float32 or t.dim() != 3 or t.shape != some.shape for t in maps):
        raise ValueError("pool_bins: float32 [B*N, H, W] maps of one shape expected")
    (dlo, dbin, dn), rc = bin_constants(grid_config)
    if rcs is not None and rc is None:
        raise ValueError("pool_bins: grid_config has no 'rcs' entry")
    rlo, roff, rbin, rn = rc if rcs is not None else (0.0, 0.0, 1.0, 1)
    bn, H, W = some.shape
    ds = int(downsample)
    if ds < 1 or H % ds or W % ds:
        raise ValueError(f"pool_bins: a {H} x {W} map is not a multiple of downsample={ds}")
    shape, dev = (bn, H // ds, W // ds), some.device
    pooled = torch.empty(shape, dtype=torch.float32, device=dev) if depth is not None else None
    bins = torch.empty(shape, dtype=torch.int32, device=dev) if depth is not None else None
    cls = torch.empty(shape, dtype=torch.int32, device=dev) if rcs is not None else None
    p = lambda t: _lib.ptr(t) if t is not None else None         # noqa: E731
    rc_ = _lib.lib().rac_lss_pool_bins_fwd(p(depth), p(rcs), p(pooled), p(bins), p(cls), bn, H, W, ds, dlo, dbin, dn, rlo, roff,
                                           rbin, rn, _lib.stream_ptr())
    _lib.check(rc_, "rac_lss_pool_bins_fwd")
    return pooled, bins, cls


def radar_prior_forward(bins, rcs_class, weight, bias, D):
    """The forward launch alone (no autograd): -> prior [B*N, (D+1)+E, h, w]"""
    w2, b = weight.detach().contiguous().float(), bias.detach().contiguous().float()
    _lib.require_gpu(bins, rcs_class, w2, b, what="radar_prior")
    if bins.dtype != torch.int32 or rcs_class.dtype != torch.int32 or bins.shape != rcs_class.shape or bins.dim() != 3:
        raise ValueError("radar_prior: int32 [B*N, h, w] index maps of one shape expected")
    E, n_rcs = w2.shape[0], w2.numel() // max(w2.shape[0], 1)
    bn, h, w = bins.shape
    out = torch.empty(bn, D + 1 + E, h, w, dtype=torch.float32, device=bins.device)
    rc = _lib.lib().rac_lss_prior_fwd(_lib.ptr(bins), _lib.ptr(rcs_class), _lib.ptr(w2), _lib.ptr(b), _lib.ptr(out), bn, h * w, D, E,
                                      n_rcs, _lib.stream_ptr())
    _lib.check(rc, "rac_lss_prior_fwd")
    return out


def radar_prior_backward(grad_out, rcs_class, D, E, n_rcs):
    """The backward launch alone: grad_out [B*N, (D+1)+E, h, w] -> (grad_weight [E, n_rcs], grad_bias [E])"""
    grad_out = grad_out.contiguous().float()
    _lib.require_gpu(grad_out, rcs_class, what="radar_prior_backward")
    bn, h, w = rcs_class.shape
    gw = torch.empty(E, n_rcs, dtype=torch.float32, device=grad_out.device)
    gb = torch.empty(E, dtype=torch.float32, device=grad_out.device)
    work = torch.empty(PRIOR_BWD_SEGMENTS * E * (n_rcs + 1), dtype=torch.float32, device=grad_out.device)
    rc = _lib.lib().rac_lss_prior_bwd(_lib.ptr(grad_out), _lib.ptr(rcs_class), _lib.ptr(work), _lib.ptr(gw), _lib.ptr(gb), bn, h * w, D, E,
                                      n_rcs, _lib.stream_ptr())
    _lib.check(rc, "rac_lss_prior_bwd")
    return gw, gb


class RadarPriorFunction(torch.autograd.Function):
    """(bins, rcs_class int32 [B*N,h,w], weight [E, n_rcs(,1,1)], bias [E], D) -> prior [B*N, (D+1)+E, h, w]"""

    @staticmethod
    def forward(ctx, bins, rcs_class, weight, bias, D):
        out = radar_prior_forward(bins, rcs_class, weight, bias, D)
        ctx.save_for_backward(rcs_class)
        ctx.dims = (D, weight.shape[0], weight.numel() // weight.shape[0], weight.shape)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (rcs_class,) = ctx.saved_tensors
        D, E, n_rcs, wshape = ctx.dims
        gw, gb = radar_prior_backward(grad_out, rcs_class, D, E, n_rcs)
        return None, None, gw.view(wshape), gb, None


def radar_prior(bins, rcs_class, weight, bias, D):
    """The tensor ``DepthNet.forward`` concatenates behind its features: channels 0..D the one-hot radar depth grid, channels
    D+1.. the RCS embedding.  Differentiable in ``weight`` and ``bias``."""
    if not _on_device(bins, rcs_class, weight):
        return radar_prior_torch(bins, rcs_class, weight, bias, D)
    return RadarPriorFunction.apply(bins, rcs_class, weight, bias, int(D))


def depth_loss_forward(depth_preds, bins, alpha=0.25, gamma=2.0, weight=3.0, pixel_loss=None):
    """The forward launches alone (no autograd): -> (loss [1], grad_unit [B*N,D,h,w], scale [1]); ``depth_loss_backward`` turns
    the last two into the gradient.  ``pixel_loss``: a float32 [B*N, h, w] tensor to receive every pixel's own term, or None."""
    _lib.require_gpu(depth_preds, bins, what="depth_loss")
    if depth_preds.dtype != torch.float32 or bins.dtype != torch.int32 or depth_preds.dim() != 4 \
            or bins.shape != depth_preds.shape[:1] + depth_preds.shape[2:]:
        raise ValueError("depth_loss: float32 logits [B*N, D, h, w] and int32 labels [B*N, h, w] expected")
    bn, D, h, w = depth_preds.shape
    dev = depth_preds.device
    partial = torch.empty(-(-bn * h * w // 64), 2, dtype=torch.float32, device=dev)
    grad_unit = torch.empty_like(depth_preds)
    loss, scale = torch.empty(1, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.float32, device=dev)
    rc = _lib.lib().rac_lss_depth_loss_fwd(_lib.ptr(depth_preds), _lib.ptr(bins), _lib.ptr(partial), _lib.ptr(grad_unit),
                                           _lib.ptr(pixel_loss) if pixel_loss is not None else None, _lib.ptr(loss), _lib.ptr(scale), bn, D, h * w, alpha, gamma, weight, _lib.stream_ptr())
    _lib.check(rc, "rac_lss_depth_loss_fwd")
    return loss, grad_unit, scale


def depth_loss_backward(grad_loss, grad_unit, scale):
    grad_loss = grad_loss.reshape(1).contiguous().float()
    out = torch.empty_like(grad_unit)
    rc = _lib.lib().rac_lss_depth_loss_bwd(_lib.ptr(grad_unit), _lib.ptr(scale), _lib.ptr(grad_loss), _lib.ptr(out), grad_unit.numel(),
                                           _lib.stream_ptr())
    _lib.check(rc, "rac_lss_depth_loss_bwd")
    return out


class DepthLossFunction(torch.autograd.Function):
    """(logits [B*N,D,h,w], labels int32 [B*N,h,w], alpha, gamma, weight) -> loss (0-dim)"""

    @staticmethod
    def forward(ctx, depth_preds, bins, alpha, gamma, weight):
        loss, grad_unit, scale = depth_loss_forward(depth_preds, bins, alpha, gamma, weight)
        ctx.save_for_backward(grad_unit, scale)
        return loss.view(())

    @staticmethod
    def backward(ctx, grad_loss):
        grad_unit, scale = ctx.saved_tensors
        return depth_loss_backward(grad_loss, grad_unit, scale), None, None, None, None


def depth_loss(depth_preds, bins, alpha=0.25, gamma=2.0, weight=3.0):
    """``weight * sum of the foreground pixels' focal terms / max(1, foreground pixels)``: depth logits [B*N, D, h, w] against
    the bin labels of ``pool_bins`` (foreground: label < D).  A 0-dim tensor; differentiable in the logits."""
    if not _on_device(depth_preds, bins):
        return depth_loss_torch(depth_preds, bins, alpha, gamma, weight)
    return DepthLossFunction.apply(depth_preds.contiguous(), bins, float(alpha), float(gamma), float(weight))


# ------------------------------------------------------------------------------------------------------------ module
def _cells_torch(img2lidar, frustum, grid, n_cams):
    """get_lidar_coor and the cell of every frustum point in torch (:112-170), float32: int64 [B*N*D*H*W], -1 if dropped."""
    D, H, W, _ = frustum.shape
    pts = torch.cat((frustum, torch.ones_like(frustum[..., :1])), -1)
    pts = torch.cat((pts[..., :2] * torch.maximum(pts[..., 2:3], torch.ones_like(pts[..., 2:3]) * 1e-5), pts[..., 2:]), -1)
    xyz = torch.matmul(img2lidar.view(-1, 1, 1, 1, 4, 4), pts.view(1, D, H, W, 4, 1)).squeeze(-1)[..., :3]
    idx = ((xyz - torch.tensor(grid.lower)) / torch.tensor(grid.interval)).long()
    X, Y, Z = grid.size
    kept = ((idx >= 0) & (idx < torch.tensor([X, Y, Z]))).all(-1)
    b = (torch.arange(xyz.shape[0]) // n_cams).view(-1, 1, 1, 1)
    cell = ((b * Z + idx[..., 2]) * Y + idx[..., 1]) * X + idx[..., 0]
    return torch.where(kept, cell, torch.full_like(cell, -1)).reshape(-1)


def _splat_torch(depth_digit, tran_feat, cells, grid, batch):
    """bev [B, Z*C, Y, X] (channel z*C + c): softmax, lift, and the sum per cell in ascending point order (``index_add``)."""
    X, Y, Z = grid.size
    bn, D, H, W = depth_digit.shape
    C = tran_feat.shape[1]
    p = depth_digit.softmax(dim=1).reshape(-1)
    feat = tran_feat.permute(0, 2, 3, 1).reshape(bn * H * W, C)
    rd = torch.nonzero(cells >= 0).flatten()
    rf = (rd // (D * H * W)) * (H * W) + rd % (H * W)
    out = torch.zeros(batch * Z * Y * X, C, dtype=p.dtype).index_add(0, cells[rd].long(), p[rd].unsqueeze(1) * feat[rf])
    return out.view(batch, Z, Y, X, C).permute(0, 1, 4, 2, 3).reshape(batch, Z * C, Y, X)


class LSSViewTransformerBEVDepth_racformer(LSSViewTransformer_racformer):
    """The reference's module (:572-699) with its constructor arguments, method signatures and state-dict keys (``frustum``,
    ``depth_net.*``, ``rcs_embedding.weight``, ``rcs_embedding.bias``).  ``depth_net``: the module to run between the priors and
    the view transform, any ``nn.Module`` with the reference's ``forward(x, radar_feats, rcs_embedding, mlp_input)`` returning
    [B*N, D + out_channels, h, w].  ``from_config`` builds this package's ``DepthNet(in_channels, in_channels, out_channels, D,
    **depthnet_cfg)`` as the reference's constructor does (:574-578); with it, on its HIP route, ``forward`` hands the index maps
    and the embedding to ``DepthNet.forward_fused`` and ``rac_lss_prior_fwd`` is skipped.  Any other ``depth_net`` gets the dense
    prior tensor.

    On device tensors every method runs the HIP kernels; on CPU tensors the torch restatement (the view transform included)."""

    def __init__(self, loss_depth_weight=3.0, loss_reg_depth_weight=1.0, depthnet_cfg=dict(), depth_net=None, **kwargs):
        super().__init__(**kwargs)
        if not isinstance(depth_net, nn.Module):
            raise TypeError("LSSViewTransformerBEVDepth_racformer: pass the DepthNet as depth_net=<nn.Module>")
        if "rcs" not in self.grid_config:
            raise ValueError("LSSViewTransformerBEVDepth_racformer: grid_config needs an 'rcs' entry (lower, upper, bins)")
        self.loss_depth_weight = loss_depth_weight
        self.depthnet_cfg = depthnet_cfg
        self.depth_net = depth_net
        self.n_rcs = int(self.grid_config["rcs"][2])
        self.rcs_embedding = nn.Conv2d(self.n_rcs, 32, kernel_size=1, padding=0)
        self.focal_alpha, self.focal_gamma = 0.25, 2.0

    @classmethod
    def from_config(cls, depthnet_cfg=dict(), **kwargs):
        """The reference's constructor call (:574-578): the keyword arguments of this class without ``depth_net``, which is built
        as ``DepthNet(in_channels, in_channels, out_channels, D, **depthnet_cfg)``."""
        if "depth_net" in kwargs:
            raise TypeError("LSSViewTransformerBEVDepth_racformer.from_config builds the depth_net itself")
        in_channels, out_channels = kwargs.get("in_channels", 512), kwargs.get("out_channels", 64)    # (the base class's defaults)
        net = DepthNet(in_channels, in_channels, out_channels, int(kwargs["grid_config"]["depth"][2]), **depthnet_cfg)
        return cls(depthnet_cfg=depthnet_cfg, depth_net=net, **kwargs)

    def get_mlp_input(self, img_metas):
        """[B, N*T, 9] float32 on the module's device: the upper-left 3x3 of every inverted ``lidar2img`` (:584-591)."""
        inv = np.linalg.inv(np.stack([meta["lidar2img"] for meta in img_metas]))
        mlp_input = torch.from_numpy(inv[:, :, :3, :3]).to(torch.float32).contiguous().view(len(img_metas), -1, 9)
        return mlp_input.to(self.frustum.device)

    def _maps(self, t):
        B, N, H, W = t.shape
        return t.reshape(B * N, H, W).contiguous().float()

    def get_downsampled_depth(self, depths, downsample):
        """depths [B, N, H, W] -> (bin indices int64 [B*N, h, w], pooled depths [B*N, h, w])"""
        downsample = self.downsample if downsample <= 0 else downsample
        pooled, bins, _ = pool_bins(self._maps(depths), None, self.grid_config, downsample)
        return bins.long(), pooled

    def get_downsampled_rcs(self, rcs, downsample):
        """rcs [B, N, H, W] -> the float one-hot [B*N, h, w, n_rcs] (all zero for class -1).  For drop-in use: ``forward``
        works on the class map and never builds this tensor."""
        downsample = self.downsample if downsample <= 0 else downsample
        _, _, cls = pool_bins(None, self._maps(rcs), self.grid_config, downsample)
        return F.one_hot(cls.long() + 1, num_classes=self.n_rcs + 1)[..., 1:].float()

    def get_depth_loss(self, depth_labels, depth_preds, downsample=0):
        """depth_labels [B, N, H, W] (the lidar depth map), depth_preds [B*N, D, h, w] -> loss_depth (0-dim)"""
        downsample = self.downsample if downsample <= 0 else downsample
        _, bins, _ = pool_bins(self._maps(depth_labels), None, self.grid_config, downsample)
        if depth_preds.dtype != torch.float64:           # (force_fp32; a float64 CPU run stays float64)
            depth_preds = depth_preds.float()
        return depth_loss(depth_preds, bins, self.focal_alpha, self.focal_gamma, self.loss_depth_weight)

    def view_transform_core(self, x, depth_digit, tran_feat, img_metas):
        if depth_digit.is_cuda:
            return super().view_transform_core(x, depth_digit, tran_feat, img_metas)
        batch = len(img_metas)
        if self.accelerate:
            cells = self.ranks.cells
        else:
            cells = _cells_torch(img2lidar_from_metas(img_metas), self.frustum.data, self.grid, depth_digit.shape[0] // batch)
        return _splat_torch(depth_digit, tran_feat, cells, self.grid, batch), depth_digit

    def view_transform(self, x, depth_digit, tran_feat, img_metas):
        if depth_digit.is_cuda:
            return super().view_transform(x, depth_digit, tran_feat, img_metas)
        if self.accelerate and self.initial_flag:
            cells = _cells_torch(img2lidar_from_metas(img_metas), self.frustum.data, self.grid, depth_digit.shape[0] // len(img_metas))
            self.ranks = RankTables(cells, None, None, None, None, None, None)
            self.initial_flag = False
        return self.view_transform_core(x, depth_digit, tran_feat, img_metas)

    def forward(self, x, radar_depth, radar_rcs, img_metas, mlp_input):
        """x [B, N, C_in, h, w], radar_depth / radar_rcs [B, N, H, W] -> (bev_feat [B, Z*C, Y, X], depth_digit [B*N, D, h, w])"""
        B, N, C, H, W = x.shape
        x = x.reshape(B * N, C, H, W)
        _, rad_inds, rcs_class = pool_bins(self._maps(radar_depth), self._maps(radar_rcs), self.grid_config, self.downsample)
        emb = self.rcs_embedding
        if isinstance(self.depth_net, DepthNet) and self.depth_net.hip_route(x, mlp_input, rad_inds, rcs_class, emb.weight, emb.bias):
            # this package's DepthNet on its kernels: the prior tensor is two table lookups inside dep_proj, never built
            x = self.depth_net.forward_fused(x, rad_inds, rcs_class, emb.weight, emb.bias, mlp_input)
        else:
            prior = radar_prior(rad_inds, rcs_class, emb.weight, emb.bias, self.D)
            x = self.depth_net(x, prior[:, :self.D + 1], prior[:, self.D + 1:], mlp_input)
        depth_digit = x[:, :self.D, ...]
        tran_feat = x[:, self.D:self.D + self.out_channels, ...]
        return self.view_transform(x, depth_digit, tran_feat, img_metas)
