"""The radar branch in front of the decoder: raw radar clouds ``[n, 7]`` to ``radar_bev_feats [B, T, 256, H, W]`` -- the
reference's ``RaCFormer.extract_pts_feat`` (models/racformer.py:130-177: mmcv's hard ``Voxelization``, mmdet3d's
``PillarFeatureNet`` and ``PointPillarsScatter``, then the three ``ConvModule`` s of ``radar_bev_conv``, :81-99), stacked over the
frames (:333-342).  Inference runs on the HIP kernels of ``csrc/radar_pillars.hip`` (``rac_pillar_*``),
``csrc/conv_direct.hip`` (modes ``RAC_CD_IMAGE_RELU`` / ``RAC_CD_F32_CF_RELU``) and ``csrc/conv3x3.hip``
(``rac_conv3x3_relu_cf_fwd``); nothing is read back and every launch is sized by an upper bound, so the branch can be captured
into a graph; two runs give the same bits.

Training (opt-in: ``RadarPillarEncoder.fused_grad = True`` and ``.train()``; off, training-mode BatchNorm raises as before): the
reference runs ``extract_pts_feat`` on frame 0 in training mode under autograd (:316-331), frames 1 .. T-1 in eval mode under
``no_grad`` on the statistics frame 0 has just updated.  ``extract_pts_feat`` then is one ``torch.autograd.Function``
(``_RadarTrainCore``): voxelize (cap ``max_voxels[0]``), the PFN layer on BATCH statistics over all M * P rows of the call into an
fp32 canvas (``rac_pillar_train_fwd``), and three times ``resnet.conv_fwd`` on the raw weight + batch-stat BatchNorm2d + ReLU
(``rac_bn_train_*``, csrc/batchnorm_train.hip); the kernels update running_mean / running_var / num_batches_tracked on the device
through raw pointers, so the caches keyed on ``_version`` (``_folded``, ``_packed``) are dropped explicitly.  The backward returns
gradients for linear.weight, the PFN norm.weight / norm.bias and every layer's conv.weight / bn.weight / bn.bias, skipping launches
nothing asks for; float64 sums in fixed orders, no float atomics: two runs give the same bits.  With the weight packs cached a
forward + backward of ``extract_pts_feat`` reads nothing back (re-packing a changed weight reads its absmax, and frames 1 .. T-1 of
``forward`` re-fold the eval route's weights on the new statistics, which reads their norms, as after any parameter change).
No pillar at all: zero canvas, PFN statistics untouched, zero PFN gradients.  CPU tensors and ``fused=False`` take the torch
modules in training mode under autograd (the comparator).  ``RaCFormer.forward_train`` (detector.py) drives this route: setting the
detector's ``fused_grad`` sets this one.  Not here: gradients to the points (voxelization is no_grad in the reference too).

mmcv and mmdet3d are not importable here: the semantics below restate their documented behaviour (mmcv 1.6.0, mmdet3d 1.0.0rc6)
under the f8 configuration.  Three quirks of the reference are KEPT:
  * padded rows in the max: a pillar with fewer than ``max_num_points`` points still feeds its zeroed rows through Linear /
    BatchNorm / ReLU / max, so no channel of it goes below ``relu(beta - running_mean * gamma / sqrt(running_var + eps))``;
  * z is treated as 0: the reference zeroes column 2 of the caller's tensors (:135-137); here the inputs are NOT mutated, the
    packed copy of the clouds has its z column zeroed (``RadarPillarEncoder``; ``hard_voxelize`` itself takes z as given);
  * the deterministic voxel order: the config's ``deterministic=False`` lets mmcv's GPU path keep an arbitrary subset of
    ``max_num_points`` points and an arbitrary pillar order; this is the ONE deterministic definition (mmcv's CPU path and its
    ``deterministic=True``): points in input order, pillars in order of their first point -- one of the legal outcomes.
Three cases the reference breaks on are DEFINED here:
  * exactly one pillar in a call (the reference's ``.squeeze()`` drops the pillar dimension) works like any other count;
  * no pillar at all (the reference's ``coors[-1, 0]`` fails): an empty cloud yields the convolution stack's response to an
    all-zero canvas;
  * the batch size comes from the caller (the number of clouds passed), not from the last pillar's sample index.

Tensors that are not on the GPU, and ``fused=False``, take a vectorised torch route (stable sort by cell for the voxelization,
``nn`` layers for the rest): the CPU path and the benchmark's baseline (tools/radar_pillars_bench.py).
Out of scope: dynamic voxelization; training-mode BatchNorm without the ``fused_grad`` switch (raises).
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib

VoxelGeom = namedtuple("VoxelGeom", "lo vs grid")              # (x, y, z) each: float32 values as Python floats; cells as ints
PackedVoxels = namedtuple("PackedVoxels", "voxels coors num_points counts amax offsets n_clouds")


def voxel_geom(voxel_size, point_cloud_range):
    """``VoxelGeom`` through float32, as mmcv's ``Voxelization.__init__``: grid = round((hi - lo) / voxel_size)."""
    r = np.asarray(point_cloud_range, dtype=np.float32)
    vs = np.asarray(voxel_size, dtype=np.float32)
    grid = np.round((r[3:] - r[:3]) / vs).astype(np.int64)
    return VoxelGeom(tuple(float(v) for v in r[:3]), tuple(float(v) for v in vs), tuple(int(v) for v in grid))


def pack_clouds(clouds, zero_z=False, pinned=False):
    """list of [n_i, C] float32 clouds -> (points [sum n_i, C] -- a new tensor, the inputs stay as they are --,
    cloud_offsets int32 [len + 1] on the same device).  The offsets come from the shapes: an upload, not a read-back;
    ``pinned`` uploads them from pinned memory without the host waiting for the copy."""
    if len(clouds) == 0:
        raise ValueError("pack_clouds: no clouds")
    C = clouds[0].shape[1]
    for c in clouds:
        if c.dim() != 2 or c.shape[1] != C or c.dtype != torch.float32:
            raise ValueError("pack_clouds: every cloud has to be a float32 [n, C] tensor of one width")
    points = torch.cat([c.detach() for c in clouds], dim=0).contiguous()
    if zero_z:
        points[:, 2] = 0
    off = np.zeros(len(clouds) + 1, dtype=np.int32)
    off[1:] = np.cumsum([c.shape[0] for c in clouds])
    off = torch.from_numpy(off)
    if pinned and points.is_cuda:                           # (from pinned memory, in stream order: the host does not wait for it)
        return points, off.pin_memory().to(points.device, non_blocking=True)
    return points, off.to(points.device)


# ------------------------------------------------------------------------------------------------ voxelization
def voxelize_packed(points, cloud_offsets, geom, max_num_points, max_voxels):
    """rac_pillar_voxelize_fwd: packed clouds -> ``PackedVoxels`` (untrimmed, nothing read back): voxels [N, P, C], coors [N, 4] =
    (cloud, z, y, x) with -1 padding, num_points [N] with 0 padding, counts [n_clouds], amax [1]; pillar i of cloud c is row
    ``cloud_offsets[c] + i``."""
    _lib.require_gpu(points, cloud_offsets, what="voxelize_packed")
    if points.dtype != torch.float32 or cloud_offsets.dtype != torch.int32 or points.dim() != 2:
        raise TypeError("voxelize_packed: float32 points [N, C] and int32 offsets expected")
    n, C = points.shape
    n_clouds = cloud_offsets.numel() - 1
    dev = points.device
    cells = geom.grid[0] * geom.grid[1] * geom.grid[2]
    voxels = torch.empty(n, max_num_points, C, dtype=torch.float32, device=dev)
    coors = torch.empty(n, 4, dtype=torch.int32, device=dev)
    num = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.empty(max(n_clouds, 1), dtype=torch.int32, device=dev)
    amax = torch.empty(1, dtype=torch.float32, device=dev)
    work = torch.empty(2 * n_clouds * cells + n + 1, dtype=torch.int32, device=dev)
    rc = _lib.lib().rac_pillar_voxelize_fwd(_lib.ptr(points), _lib.ptr(cloud_offsets), _lib.ptr(voxels), _lib.ptr(coors), _lib.ptr(num),
                                            _lib.ptr(counts), _lib.ptr(amax), _lib.ptr(work), n, n_clouds, C, *geom.lo, *geom.vs,
                                            *geom.grid, int(max_num_points), int(max_voxels), _lib.stream_ptr())
    _lib.check(rc, "rac_pillar_voxelize_fwd")
    return PackedVoxels(voxels, coors, num, counts[:n_clouds], amax, cloud_offsets, n_clouds)


def trim_packed(pv):
    """``PackedVoxels`` -> (voxels [M, P, C], coors [M, 4], num_points [M]) of the M real pillars, cloud after cloud: ONE
    read-back (the mask of real rows), like ``lss_rank_tables(trim=True)``."""
    keep = pv.coors[:, 0] >= 0
    return pv.voxels[keep], pv.coors[keep], pv.num_points[keep]


def _hard_voxelize_torch(points, geom, max_num_points, max_voxels):
    """The same deterministic definition in vectorised torch ops (any device): stable sort of the in-range points by cell; a
    point's slot is its position inside its cell's run, a cell's pillar index the rank of its first point."""
    n, C = points.shape
    dev = points.device
    gx, gy, gz = geom.grid
    lo, vs = points.new_tensor(geom.lo), points.new_tensor(geom.vs)
    c = torch.floor((points[:, :3] - lo) / vs)
    ok = ((c >= 0) & (c < points.new_tensor([float(g) for g in geom.grid]))).all(dim=1)
    idx = torch.nonzero(ok).squeeze(1)
    ci = c[idx].long()
    key = (ci[:, 2] * gy + ci[:, 1]) * gx + ci[:, 0]
    order = torch.argsort(key, stable=True)
    ks = key[order]
    new = torch.ones_like(ks, dtype=torch.bool)
    new[1:] = ks[1:] != ks[:-1]
    starts = torch.nonzero(new).squeeze(1)
    gid = torch.cumsum(new.long(), 0) - 1
    slot = torch.arange(ks.numel(), device=dev) - starts[gid]
    first_pos = order[starts]                                   # (stable sort: a run starts with the cell's first point)
    rank = torch.empty_like(first_pos)
    rank[torch.argsort(first_pos)] = torch.arange(first_pos.numel(), device=dev)
    pillar = rank[gid]
    keep = (pillar < max_voxels) & (slot < max_num_points)
    M = min(int(starts.numel()), int(max_voxels))
    voxels = points.new_zeros(M, max_num_points, C)
    voxels[pillar[keep], slot[keep]] = points[idx[order[keep]]]
    num = torch.zeros(M, dtype=torch.int32, device=dev)
    coors = torch.zeros(M, 3, dtype=torch.int32, device=dev)
    live = rank < max_voxels
    lengths = torch.diff(torch.cat([starts, starts.new_tensor([ks.numel()])]))
    num[rank[live]] = lengths[live].clamp(max=max_num_points).int()
    cell = ks[starts][live]
    coors[rank[live]] = torch.stack([cell // (gx * gy), (cell // gx) % gy, cell % gx], dim=1).int()
    return voxels, coors, num


def hard_voxelize(points, voxel_size, point_cloud_range, max_num_points, max_voxels, fused=True):
    """Drop-in for mmcv's ``Voxelization.forward`` (hard voxelization) on one cloud ``[n, C]``:
    -> (voxels [M, max_num_points, C] zero-padded, coors [M, 3] int32 = (z, y, x), num_points [M] int32), in the deterministic
    order of the module docstring.  On the GPU the kernels run and the result is trimmed to M by one read-back."""
    geom = voxel_geom(voxel_size, point_cloud_range)
    points = points.detach()
    if not (fused and points.is_cuda):
        return _hard_voxelize_torch(points.float(), geom, int(max_num_points), int(max_voxels))
    pts, off = pack_clouds([points.contiguous()])
    voxels, coors, num = trim_packed(voxelize_packed(pts, off, geom, max_num_points, max_voxels))
    return voxels, coors[:, 1:].contiguous(), num


class Voxelization(nn.Module):
    """mmcv's ``Voxelization`` with the reference config's constructor arguments (hard voxelization only: ``max_num_points`` > 0).
    ``max_voxels`` = (training, testing); ``deterministic`` is accepted and ignored: the order is always the deterministic one."""

    def __init__(self, voxel_size, point_cloud_range, max_num_points, max_voxels=20000, deterministic=True, fused=True):
        super().__init__()
        if max_num_points <= 0:
            raise NotImplementedError("Voxelization: dynamic voxelization (max_num_points <= 0) is out of scope")
        self.voxel_size, self.point_cloud_range = list(voxel_size), list(point_cloud_range)
        self.max_num_points = int(max_num_points)
        self.max_voxels = tuple(max_voxels) if isinstance(max_voxels, (tuple, list)) else (max_voxels, max_voxels)
        self.geom = voxel_geom(voxel_size, point_cloud_range)
        self.grid_size = torch.tensor(self.geom.grid)
        self.fused = fused

    def cap(self):
        return int(self.max_voxels[0] if self.training else self.max_voxels[1])

    def forward(self, points):
        return hard_voxelize(points, self.voxel_size, self.point_cloud_range, self.max_num_points, self.cap(), fused=self.fused)


# ------------------------------------------------------------------------------------------------ pillar features
def fold_bn(weight, bn):
    """(weight [out, ...], BatchNorm with running statistics) -> (weight * g, shift) with g = gamma / sqrt(var + eps) per output
    channel and shift = beta - mean * g; folded in float64, rounded to float32 once."""
    g = bn.weight.detach().double() / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    shift = bn.bias.detach().double() - bn.running_mean.detach().double() * g
    w = weight.detach().double() * g.view(-1, *([1] * (weight.dim() - 1)))
    return w.float().contiguous(), shift.float().contiguous()


def _no_training(module, what):
    if any(m.training for m in module.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)):
        raise RuntimeError(f"{what}: training-mode BatchNorm (batch statistics over ragged pillar rows, backward) is out of scope; "
                           "call .eval() -- this branch runs forward only, on running statistics")


def _param_sig(module):
    return tuple((t.data_ptr(), t._version, str(t.device)) for t in list(module.parameters()) + list(module.buffers()))


# ------------------------------------------------------------------------------------------------ training-mode BatchNorm
def _running_args(bn):
    """(running_mean, running_var, num_batches_tracked pointers or three None, momentum) of a BatchNorm for the training kernels,
    which update the buffers in place on the device (their ``_version`` does not move)."""
    if bn.running_mean is None or not bn.track_running_stats:
        return None, None, None, 0.0
    if bn.momentum is None:
        raise NotImplementedError("training-mode BatchNorm in HIP: momentum=None (cumulative average) is not implemented")
    if bn.num_batches_tracked.dtype != torch.int64:
        raise TypeError("training-mode BatchNorm in HIP: num_batches_tracked has to be int64")
    _lib.require_gpu(bn.running_mean, bn.running_var, bn.num_batches_tracked, what="bn_train_stats")
    return _lib.ptr(bn.running_mean), _lib.ptr(bn.running_var), _lib.ptr(bn.num_batches_tracked), float(bn.momentum)


def _bn_maps(what, *tensors):
    _lib.require_gpu(*tensors, what=what)
    x = tensors[0]
    if x.dim() < 3 or any(t.dtype != torch.float32 or t.shape != x.shape for t in tensors):
        raise RuntimeError(f"{what}: contiguous float32 [N, C, ...] maps of one shape expected")
    n, c = x.shape[:2]
    return n, c, x.numel() // max(n * c, 1)


def bn_chunks(n, hw):
    """Partial sums per channel of the training-mode BatchNorm kernels for n maps of hw pixels (chunks of 4096 values)."""
    return -(-n * hw // 4096)


def bn_train_stats(x, bn=None, eps=1e-5):
    """x float32 device [N, C, H, W] -> (mean [C], invstd [C]) over N * H * W (rac_bn_train_stats_fwd); with ``bn`` (an
    ``nn.BatchNorm2d``: its eps and momentum) the running statistics are updated as its training-mode forward does."""
    n, c, hw = _bn_maps("bn_train_stats", x)
    running = _running_args(bn) if bn is not None else (None, None, None, 0.0)
    mean, invstd = torch.empty(c, dtype=torch.float32, device=x.device), torch.empty(c, dtype=torch.float32, device=x.device)
    work = torch.empty(c * bn_chunks(n, hw) * 2, dtype=torch.float64, device=x.device)
    rc = _lib.lib().rac_bn_train_stats_fwd(_lib.ptr(x), _lib.ptr(work), _lib.ptr(mean), _lib.ptr(invstd), *running[:3], n, c, hw,
                                           float(bn.eps if bn is not None else eps), running[3], _lib.stream_ptr())
    _lib.check(rc, "rac_bn_train_stats_fwd")
    return mean, invstd


def bn_train_apply(x, mean, invstd, gamma, beta, relu=True):
    """[relu]((x - mean) * invstd * gamma + beta) per channel (rac_bn_train_apply_fwd)."""
    n, c, hw = _bn_maps("bn_train_apply", x)
    gamma, beta = gamma.detach(), beta.detach()
    _lib.require_gpu(mean, invstd, gamma, beta, what="bn_train_apply")
    y = torch.empty_like(x)
    rc = _lib.lib().rac_bn_train_apply_fwd(_lib.ptr(x), _lib.ptr(mean), _lib.ptr(invstd), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(y), n, c,
                                           hw, int(bool(relu)), _lib.stream_ptr())
    _lib.check(rc, "rac_bn_train_apply_fwd")
    return y


def bn_train_bwd(g, x, y, mean, invstd, gamma, need_dx=True):
    """g = dL/dy, the BatchNorm's input x, its post-ReLU output y (None: no ReLU decision to apply -- there was none, or
    ``conv_dgrad``'s mask already applied it) -> (dgamma [C], dbeta [C], dx or None) (rac_bn_train_bwd)."""
    n, c, hw = _bn_maps("bn_train_bwd", g, x, *([y] if y is not None else []))
    gamma = gamma.detach()
    _lib.require_gpu(mean, invstd, gamma, what="bn_train_bwd")
    dgamma, dbeta = torch.empty(c, dtype=torch.float32, device=x.device), torch.empty(c, dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x) if need_dx else None
    work = torch.empty(c * bn_chunks(n, hw) * 2, dtype=torch.float64, device=x.device)
    rc = _lib.lib().rac_bn_train_bwd(_lib.ptr(g), _lib.ptr(x), _lib.ptr(y) if y is not None else None, _lib.ptr(mean), _lib.ptr(invstd),
                                     _lib.ptr(gamma), _lib.ptr(work), _lib.ptr(dgamma), _lib.ptr(dbeta), _lib.ptr(dx) if need_dx else None,
                                     n, c, hw, _lib.stream_ptr())
    _lib.check(rc, "rac_bn_train_bwd")
    return dgamma, dbeta, dx


class PFNLayer(nn.Module):
    def __init__(self, in_channels, out_channels, eps=1e-3, momentum=0.01):
        super().__init__()
        self.linear = nn.Linear(in_channels, out_channels, bias=False)
        self.norm = nn.BatchNorm1d(out_channels, eps=eps, momentum=momentum)

    def forward(self, inputs):
        x = self.linear(inputs)
        x = self.norm(x.transpose(1, 2).contiguous()).transpose(1, 2).contiguous()
        return torch.relu(x).max(dim=1, keepdim=True)[0]


class PillarFeatureNet(nn.Module):
    """mmdet3d's ``PillarFeatureNet`` for the reference configuration: one PFN layer, cluster and voxel centres, no distance,
    ``legacy=False``, BatchNorm1d(eps=1e-3).  Parameter names as in mmdet3d (``pfn_layers.0.linear.weight``,
    ``pfn_layers.0.norm.*``).  ``forward(features [M, P, C], num_points [M], coors [M, 4] = (sample, z, y, x)) -> [M, 64]``."""

    def __init__(self, in_channels=4, feat_channels=(64,), with_distance=False, with_cluster_center=True, with_voxel_center=True,
                 voxel_size=(0.2, 0.2, 4), point_cloud_range=(0, -40, -3, 70.4, 40, 1), norm_cfg=None, mode='max', legacy=False,
                 fused=True):
        super().__init__()
        feat_channels = list(feat_channels)
        if with_distance or not with_cluster_center or not with_voxel_center or legacy or mode != 'max' or len(feat_channels) != 1:
            raise NotImplementedError("PillarFeatureNet: built for one PFN layer with cluster and voxel centres, no distance, "
                                      "legacy=False, mode='max' (the reference configuration)")
        norm_cfg = norm_cfg or dict(type='BN1d', eps=1e-3, momentum=0.01)
        self.in_channels = int(in_channels)
        self.pfn_layers = nn.ModuleList([PFNLayer(in_channels + 6, feat_channels[0], eps=norm_cfg.get('eps', 1e-3),
                                                  momentum=norm_cfg.get('momentum', 0.01))])
        self.vx, self.vy, self.vz = (float(v) for v in voxel_size)
        self.x_offset = self.vx / 2 + point_cloud_range[0]
        self.y_offset = self.vy / 2 + point_cloud_range[1]
        self.z_offset = self.vz / 2 + point_cloud_range[2]
        self.point_cloud_range = list(point_cloud_range)
        self.fused = fused
        self._folded = None

    def folded(self):
        """(wt [C + 6, 64] = the Linear's weight with the BatchNorm folded in, transposed; shift [64]; max-row L1 norm; largest
        positive shift), cached per parameter version."""
        sig = _param_sig(self)
        if self._folded is None or self._folded[0] != sig:
            layer = self.pfn_layers[0]
            w, shift = fold_bn(layer.linear.weight, layer.norm)
            self._folded = (sig, w.t().contiguous(), shift, float(w.abs().sum(dim=1).max()), max(float(shift.max()), 0.0))
        return self._folded[1:]

    def image_bound(self):
        """(mul, add): the pillar features are bounded by mul * A + add, A = max |value| of the in-range points: every decorated
        feature is at most 2 A + R in magnitude (raw <= A, xyz - mean <= 2 A, xyz - centre <= A + R with R the range's largest
        |coordinate|), so a channel is at most L1 * (2 A + R) + shift."""
        _, _, l1, smax = self.folded()
        R = max(abs(float(v)) for v in self.point_cloud_range)
        return 2.0 * l1, l1 * R + smax

    def encode(self, voxels, coors, num_points, n_clouds, H, W, amax=None, canvas=None, image=None, feats=None):
        """rac_pillar_encode_fwd on (packed or trimmed) pillar rows into any of the three destinations."""
        _no_training(self, "PillarFeatureNet")
        wt, shift, _, _ = self.folded()
        mul, add = self.image_bound()
        n_rows, P, C = voxels.shape
        if C != self.in_channels or wt.shape[1] != 64:
            raise ValueError(f"PillarFeatureNet: {C}-wide points for in_channels={self.in_channels}; 64 feature channels expected")
        tensors = [t for t in (voxels, coors, num_points, wt, shift, amax, canvas, image, feats) if t is not None]
        _lib.require_gpu(*tensors, what="PillarFeatureNet")
        opt = lambda t: _lib.ptr(t) if t is not None else None      # noqa: E731
        rc = _lib.lib().rac_pillar_encode_fwd(_lib.ptr(voxels), _lib.ptr(coors), _lib.ptr(num_points), _lib.ptr(wt), _lib.ptr(shift),
                                              opt(amax), mul, add, opt(canvas), opt(image), opt(feats), n_rows, int(n_clouds), C, P, 64,
                                              self.vx, self.vy, self.vz, float(np.float32(self.x_offset)),
                                              float(np.float32(self.y_offset)), float(np.float32(self.z_offset)), int(H), int(W),
                                              _lib.stream_ptr())
        _lib.check(rc, "rac_pillar_encode_fwd")

    def _geometry_args(self):
        return (self.vx, self.vy, self.vz, float(np.float32(self.x_offset)), float(np.float32(self.y_offset)),
                float(np.float32(self.z_offset)))

    def train_fwd(self, pv, H, W):
        """rac_pillar_train_fwd on packed pillar rows (``voxelize_packed``): the PFN layer on batch statistics, its BatchNorm1d's
        running statistics updated on the device -> (canvas [n_clouds, 64, H, W], what ``train_bwd`` needs)."""
        layer = self.pfn_layers[0]
        lin, bn = layer.linear, layer.norm
        n_rows, P, C = pv.voxels.shape
        dev = pv.voxels.device
        if C != self.in_channels or lin.weight.shape[0] != 64:
            raise ValueError(f"PillarFeatureNet: {C}-wide points for in_channels={self.in_channels}; 64 feature channels expected")
        wt = lin.weight.detach().t().contiguous()
        gamma, beta = bn.weight.detach(), bn.bias.detach()
        running = _running_args(bn)
        _lib.require_gpu(pv.voxels, pv.coors, pv.num_points, wt, gamma, beta, what="PillarFeatureNet.train_fwd")
        xbuf = torch.empty(n_rows, P, 64, dtype=torch.float32, device=dev)
        work = torch.empty(max(n_rows, 1) * 2 * 64, dtype=torch.float64, device=dev)
        stat = torch.empty(128, dtype=torch.float32, device=dev)
        n_total = torch.empty(1, dtype=torch.int32, device=dev)
        feats = torch.empty(n_rows, 64, dtype=torch.float32, device=dev)
        slots = torch.empty(n_rows, 64, dtype=torch.int32, device=dev)
        canvas = torch.empty(pv.n_clouds, 64, H, W, dtype=torch.float32, device=dev)
        rc = _lib.lib().rac_pillar_train_fwd(_lib.ptr(pv.voxels), _lib.ptr(pv.coors), _lib.ptr(pv.num_points), _lib.ptr(wt), _lib.ptr(gamma),
                                             _lib.ptr(beta), *running[:3], _lib.ptr(xbuf), _lib.ptr(work), _lib.ptr(stat), _lib.ptr(n_total),
                                             _lib.ptr(feats), _lib.ptr(slots), _lib.ptr(canvas), n_rows, int(pv.n_clouds), C, P, 64,
                                             float(bn.eps), running[3], *self._geometry_args(), int(H), int(W), _lib.stream_ptr())
        _lib.check(rc, "rac_pillar_train_fwd")
        self._folded = None                              # (the running statistics changed behind their version counters)
        return canvas, (pv.voxels, pv.coors, pv.num_points, xbuf, stat, n_total, feats, slots)

    def train_bwd(self, saved, dcanvas, need_dw=True):
        """rac_pillar_train_bwd: ``train_fwd``'s saved tensors and dL/dcanvas -> (dW [64, C + 6] or None, dgamma [64], dbeta [64])."""
        voxels, coors, num, xbuf, stat, n_total, feats, slots = saved
        n_rows, P, C = voxels.shape
        dev = voxels.device
        n_clouds, _, H, W = dcanvas.shape
        gamma = self.pfn_layers[0].norm.weight.detach()
        _lib.require_gpu(dcanvas, gamma, what="PillarFeatureNet.train_bwd")
        work = torch.empty(max(n_rows, 1) * 2 * 64 + (-(-n_rows // 64)) * (C + 6) * 64, dtype=torch.float64, device=dev)
        dw = torch.empty(64, C + 6, dtype=torch.float32, device=dev) if need_dw else None
        dgamma, dbeta = torch.empty(64, dtype=torch.float32, device=dev), torch.empty(64, dtype=torch.float32, device=dev)
        rc = _lib.lib().rac_pillar_train_bwd(_lib.ptr(dcanvas), _lib.ptr(voxels), _lib.ptr(coors), _lib.ptr(num), _lib.ptr(gamma),
                                             _lib.ptr(xbuf), _lib.ptr(stat), _lib.ptr(n_total), _lib.ptr(feats), _lib.ptr(slots),
                                             _lib.ptr(work), _lib.ptr(dw) if need_dw else None, _lib.ptr(dgamma), _lib.ptr(dbeta), n_rows,
                                             int(n_clouds), C, P, 64, *self._geometry_args(), int(H), int(W), _lib.stream_ptr())
        _lib.check(rc, "rac_pillar_train_bwd")
        return dw, dgamma, dbeta

    def forward(self, features, num_points, coors):
        if self.fused and features.is_cuda:
            feats = torch.zeros(features.shape[0], 64, dtype=torch.float32, device=features.device)
            self.encode(features.contiguous(), coors.int().contiguous(), num_points.int().contiguous(), 1, 1, 1, feats=feats)
            return feats
        _no_training(self, "PillarFeatureNet")
        return self.forward_torch(features, num_points, coors)

    def forward_torch(self, features, num_points, coors):
        """The same in torch ops, in the BatchNorm's own mode (running or batch statistics), under autograd if it is on."""
        dtype = features.dtype
        points_mean = features[:, :, :3].sum(dim=1, keepdim=True) / num_points.type_as(features).view(-1, 1, 1)
        f_cluster = features[:, :, :3] - points_mean
        f_center = features.new_zeros(features.shape[0], features.shape[1], 3)
        f_center[:, :, 0] = features[:, :, 0] - (coors[:, 3].to(dtype).unsqueeze(1) * self.vx + self.x_offset)
        f_center[:, :, 1] = features[:, :, 1] - (coors[:, 2].to(dtype).unsqueeze(1) * self.vy + self.y_offset)
        f_center[:, :, 2] = features[:, :, 2] - (coors[:, 1].to(dtype).unsqueeze(1) * self.vz + self.z_offset)
        x = torch.cat([features, f_cluster, f_center], dim=-1)
        mask = (torch.arange(x.shape[1], device=x.device).view(1, -1) < num_points.view(-1, 1)).type_as(x).unsqueeze(-1)
        return self.pfn_layers[0](x * mask).squeeze(1)


class PointPillarsScatter(nn.Module):
    """mmdet3d's ``PointPillarsScatter``: ``forward(voxel_features [M, C], coors [M, 4], batch_size) -> canvas [B, C, ny, nx]``,
    ``canvas[b, :, c_y, c_x] = feature``.  Pure data movement (one indexed store); the fused encoder never calls it -- its pillar
    kernel stores at the cell itself."""

    def __init__(self, in_channels, output_shape):
        super().__init__()
        self.in_channels, self.output_shape = int(in_channels), tuple(output_shape)
        self.ny, self.nx = self.output_shape

    def forward(self, voxel_features, coors, batch_size):
        canvas = voxel_features.new_zeros(int(batch_size), self.in_channels, self.ny, self.nx)
        c = coors.long()
        canvas[c[:, 0], :, c[:, 2], c[:, 3]] = voxel_features
        return canvas


class ConvModule(nn.Module):
    """mmcv's ``ConvModule`` as radar_bev_conv builds it: Conv2d(3x3, pad 1, bias=False) -> BatchNorm2d -> ReLU, submodules
    ``conv`` and ``bn``."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, 3, padding=1, bias=False)
        self.bn = nn.BatchNorm2d(out_channels)

    def forward(self, x):
        return torch.relu(self.bn(self.conv(x)))


# ------------------------------------------------------------------------------------------------ convolution stack
def pack_conv_bn(conv, bn):
    """ConvModule -> (ws, w_alpha, bias, max-row L1 norm, max |bias|) of the folded convolution, for ``conv_bn_relu``."""
    from .fused import pack_conv3x3_weight
    w, bias = fold_bn(conv.weight, bn)
    ws, alpha = pack_conv3x3_weight(w, cout=w.shape[0])
    if ws is None or w.shape[0] % 64 != 0 or w.shape[1] != 64:
        raise RuntimeError(f"radar_bev_conv: a 3x3 convolution 64 -> multiple of 64 channels with finite non-zero weights expected, "
                           f"got {tuple(w.shape)}")
    return ws, alpha, bias, float(w.abs().sum(dim=(1, 2, 3)).max()), float(bias.abs().max())


def conv_bn_relu(packed, in_img, in_scale, frames, H, W, out_img=None, out_scale=None, out=None, staged=None):
    """One layer of radar_bev_conv: relu(conv3x3(in_img) + bias) of a 64-channel activation image (scale triple ``in_scale`` =
    (amax tensor | None, mul, add)) into another activation image (``out_img`` with ``out_scale``: rac_conv_direct_fwd,
    RAC_CD_IMAGE_RELU) or into channel-first fp32 ``out`` [frames, Cout, H, W].  The fp32 destination runs on the LDS-staged kernel
    (rac_conv3x3_relu_cf_fwd) where that kernel exists, i.e. for 256 output channels -- 1.5 x faster than the direct kernel on 8
    frames of 128 x 128 (profiles/radar_pillars_f8.json) --, and on the direct kernel (RAC_CD_F32_CF_RELU) for other multiples
    of 64; ``staged`` = True / False forces one of them."""
    from .fused import conv_direct
    ws, alpha, bias, _, _ = packed
    cout = int(bias.numel())
    if out is not None and (cout == 256 if staged is None else staged):
        amax, mul, add = in_scale
        _lib.require_gpu(in_img, ws, bias, out, what="conv_bn_relu")
        rc = _lib.lib().rac_conv3x3_relu_cf_fwd(_lib.ptr(in_img), _lib.ptr(ws), _lib.ptr(bias), _lib.ptr(amax) if amax is not None else None,
                                                float(mul), float(add), float(alpha), _lib.ptr(out), frames, H, W, 64, cout,
                                                _lib.stream_ptr())
        _lib.check(rc, "rac_conv3x3_relu_cf_fwd")
        return out
    if out is not None:
        conv_direct(_lib.CD_F32_CF_RELU, frames, H, W, in_img, 2, 2, ws, alpha, cout, in_scale, bias=bias, out_f32=out)
        return out
    if cout != 64:
        raise RuntimeError("conv_bn_relu: the image destination holds 64 channels")
    conv_direct(_lib.CD_IMAGE_RELU, frames, H, W, in_img, 2, 2, ws, alpha, 64, in_scale, bias=bias, out_img=out_img, out_chunks_total=2,
                out_scale=out_scale)
    return out_img


def next_scale(scale, packed):
    """The scale triple of a layer's output image from its input's: |relu(conv + b)| <= max-row L1 * |input| + max |b|."""
    amax, mul, add = scale
    return amax, packed[3] * mul, packed[3] * add + packed[4]


# ------------------------------------------------------------------------------------------------ the branch
F8_VOXEL_LAYER = dict(max_num_points=10, voxel_size=[0.8, 0.8, 8], point_cloud_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0],
                      max_voxels=(30000, 40000), deterministic=False)


class RadarPillarEncoder(nn.Module):
    """The radar half of the detector up to the decoder's input, with the detector's submodule names: a reference checkpoint's
    ``radar_voxel_encoder.*`` and ``radar_bev_conv.{0,1,2}.{conv.weight, bn.*}`` keys load as they are.  Arguments are the
    reference config's ``radar_voxel_layer`` / ``radar_voxel_encoder`` / ``radar_middle_encoder`` dicts (``type`` keys ignored)."""

    fused_grad = False        # opt-in: in training mode extract_pts_feat runs on batch statistics under autograd (module docstring)

    def __init__(self, radar_voxel_layer=None, radar_voxel_encoder=None, radar_middle_encoder=None, embed_dims=256, fused=True):
        super().__init__()
        self._train_packed = {}
        vl = dict(radar_voxel_layer or F8_VOXEL_LAYER)
        ve = dict(radar_voxel_encoder or dict(in_channels=7, feat_channels=[64], with_distance=False, voxel_size=vl["voxel_size"],
                                              point_cloud_range=vl["point_cloud_range"], legacy=False,
                                              norm_cfg=dict(type='BN1d', eps=1e-3, momentum=0.01)))
        geom = voxel_geom(vl["voxel_size"], vl["point_cloud_range"])
        me = dict(radar_middle_encoder or dict(in_channels=64, output_shape=(geom.grid[1], geom.grid[0])))
        for d in (vl, ve, me):
            d.pop("type", None)
        self.radar_voxel_layer = Voxelization(fused=fused, **vl)
        self.radar_voxel_encoder = PillarFeatureNet(fused=fused, **ve)
        self.radar_middle_encoder = PointPillarsScatter(**me)
        c = me["in_channels"]
        self.radar_bev_conv = nn.Sequential(ConvModule(c, c), ConvModule(c, c), ConvModule(c, embed_dims))
        self.embed_dims = embed_dims
        self.fused = fused
        self._packed = None
        if self.radar_voxel_layer.geom.grid[2] != 1 or tuple(me["output_shape"]) != (geom.grid[1], geom.grid[0]):
            raise ValueError("RadarPillarEncoder: pillars (one cell in z) on the middle encoder's output_shape expected")

    def packed_convs(self):
        sig = _param_sig(self.radar_bev_conv)
        if self._packed is None or self._packed[0] != sig:
            self._packed = (sig, [pack_conv_bn(m.conv, m.bn) for m in self.radar_bev_conv])
        return self._packed[1]

    def encode_packed(self, points, cloud_offsets):
        """Packed clouds (``pack_clouds``; z as given) -> [n_clouds, 256, H, W] on the kernels: voxelize, pillar features into the
        activation image, three convolution launches.  No read-back, no allocation-size dependence on the data: capturable."""
        from .fused import act_image
        _no_training(self, "RadarPillarEncoder")
        vl, pfn = self.radar_voxel_layer, self.radar_voxel_encoder
        gx, gy, _ = vl.geom.grid
        pv = voxelize_packed(points, cloud_offsets, vl.geom, vl.max_num_points, vl.cap())
        n, dev = pv.n_clouds, points.device
        convs = self.packed_convs()
        img_a, img_b = act_image("radar_a", n, gy, gx, 64, dev), act_image("radar_b", n, gy, gx, 64, dev)
        s0 = (pv.amax,) + pfn.image_bound()
        pfn.encode(pv.voxels, pv.coors, pv.num_points, n, gy, gx, amax=pv.amax, image=img_a)
        s1 = next_scale(s0, convs[0])
        conv_bn_relu(convs[0], img_a, s0, n, gy, gx, out_img=img_b, out_scale=s1)
        s2 = next_scale(s1, convs[1])
        conv_bn_relu(convs[1], img_b, s1, n, gy, gx, out_img=img_a, out_scale=s2)
        out = torch.empty(n, self.embed_dims, gy, gx, dtype=torch.float32, device=dev)
        return conv_bn_relu(convs[2], img_a, s2, n, gy, gx, out=out)

    def canvas_packed(self, points, cloud_offsets):
        """The fp32 canvas [n_clouds, 64, H, W] alone (``PointPillarsScatter``'s result) on the kernels."""
        vl, pfn = self.radar_voxel_layer, self.radar_voxel_encoder
        gx, gy, _ = vl.geom.grid
        pv = voxelize_packed(points, cloud_offsets, vl.geom, vl.max_num_points, vl.cap())
        canvas = torch.empty(pv.n_clouds, 64, gy, gx, dtype=torch.float32, device=points.device)
        pfn.encode(pv.voxels, pv.coors, pv.num_points, pv.n_clouds, gy, gx, canvas=canvas)
        return canvas

    def radar_voxelize(self, points):
        """The reference's ``radar_voxelize`` (:153-177): per-cloud hard voxelization, concatenated, the sample index prepended
        to ``coors``.  -> (voxels, num_points, coors [M, 4])."""
        vl = self.radar_voxel_layer
        if self.fused and all(p.is_cuda for p in points):
            pts, off = pack_clouds(list(points))
            v, c, k = trim_packed(voxelize_packed(pts, off, vl.geom, vl.max_num_points, vl.cap()))
            return v, k, c
        res = [_hard_voxelize_torch(p.detach().float(), vl.geom, vl.max_num_points, vl.cap()) for p in points]
        coors = [torch.nn.functional.pad(r[1], (1, 0), value=i) for i, r in enumerate(res)]
        return torch.cat([r[0] for r in res]), torch.cat([r[2] for r in res]), torch.cat(coors)

    def _torch_route(self, clouds, train=False):
        if not train:
            _no_training(self, "RadarPillarEncoder")
        zeroed = []
        for p in clouds:
            p = p.detach().clone()
            p[:, 2] = 0
            zeroed.append(p)
        with torch.no_grad():                                  # (as in the reference: radar_voxelize is no_grad)
            voxels, num, coors = self.radar_voxelize(zeroed)
        pfn = self.radar_voxel_encoder
        if voxels.shape[0] == 0:                               # (no pillar: no batch to take statistics of)
            feats = voxels.new_zeros(0, 64)
        else:
            feats = pfn.forward_torch(voxels, num, coors) if train else pfn(voxels, num, coors)
        return self.radar_bev_conv(self.radar_middle_encoder(feats, coors, len(clouds)))

    def _clouds(self, clouds):
        """list of clouds (z as the caller has it; treated as 0, inputs untouched) -> [len, 256, H, W]"""
        with torch.no_grad():
            if self.fused and all(p.is_cuda for p in clouds):
                return self.encode_packed(*pack_clouds(list(clouds), zero_z=True))
            return self._torch_route(clouds)

    # -------------------------------------------------------------------------------------------- the training route
    def train_route(self):
        """True where ``extract_pts_feat`` trains: the switch is on and the module is in training mode."""
        return bool(self.fused_grad) and self.training

    def train_packs(self, i, transposed=False):
        """``resnet.pack_conv_weight`` (``_t``) of radar_bev_conv[i]'s RAW weight, cached per weight version (an optimizer step
        moves it); packing reads the weight's absmax on the host."""
        from . import resnet
        w = self.radar_bev_conv[i].conv.weight
        key = (i, bool(transposed))
        sig = (w.data_ptr(), w._version, str(w.device))
        hit = self._train_packed.get(key)
        if hit is None or hit[0] != sig:
            hit = self._train_packed[key] = (sig, (resnet.pack_conv_weight_t if transposed else resnet.pack_conv_weight)(w))
        return hit[1]

    def train_params(self):
        """The parameters ``_RadarTrainCore`` returns gradients for, in its order."""
        layer = self.radar_voxel_encoder.pfn_layers[0]
        out = [layer.linear.weight, layer.norm.weight, layer.norm.bias]
        for m in self.radar_bev_conv:
            out += [m.conv.weight, m.bn.weight, m.bn.bias]
        return out

    def train_forward_hip(self, points, cloud_offsets):
        """Packed clouds -> ([n_clouds, 256, H, W], the PFN layer's saved tensors, per layer (input, conv output, output, mean,
        invstd)): voxelize, the PFN layer and the three ConvModules on batch statistics; every BatchNorm's running statistics are
        updated on the device.  No read-back, no data-dependent allocation."""
        from . import resnet
        vl, pfn = self.radar_voxel_layer, self.radar_voxel_encoder
        gx, gy, _ = vl.geom.grid
        pv = voxelize_packed(points, cloud_offsets, vl.geom, vl.max_num_points, vl.cap())
        x, pfn_saved = pfn.train_fwd(pv, gy, gx)
        layers = []
        for i, m in enumerate(self.radar_bev_conv):
            z = resnet.conv_fwd(x, self.train_packs(i), None, 3, 1, relu=False)
            mean, invstd = bn_train_stats(z, m.bn)
            y = bn_train_apply(z, mean, invstd, m.bn.weight, m.bn.bias)
            layers.append((x, z, y, mean, invstd))
            x = y
        self._packed = None                                    # (the running statistics changed behind their version counters)
        return x, pfn_saved, layers

    def _clouds_train(self, clouds):
        """``_clouds`` in training mode under autograd: the HIP route on device clouds, else the torch modules."""
        if self.fused and all(p.is_cuda for p in clouds):
            points, off = pack_clouds(list(clouds), zero_z=True, pinned=True)
            return _RadarTrainCore.apply(self, points, off, *self.train_params())
        return self._torch_route(clouds, train=True)

    def extract_pts_feat(self, radar_points):
        """list over B of [n, 7] -> [B, 256, H, W]: the reference's method for one frame.  With ``fused_grad`` on and the module
        in training mode it runs on batch statistics under autograd (``_RadarTrainCore`` on device clouds)."""
        if self.train_route():
            return self._clouds_train(radar_points)
        return self._clouds(radar_points)

    def _eval_frames(self, clouds):
        """``_clouds`` with every submodule switched to eval mode for the call (the reference's frames 1 .. T-1)."""
        was = [(m, m.training) for m in self.modules()]
        self.eval()
        try:
            return self._clouds(clouds)
        finally:
            for m, t in was:
                m.training = t

    def forward(self, radar_points):
        """list over T of list over B of [n, 7] -> radar_bev_feats [B, T, 256, H, W], contiguous fp32 (the decoder's input); all
        B * T clouds go through one set of launches.  On the training route (``train_route``) frame 0 trains and frames 1 .. T-1
        run in eval mode under no_grad on the running statistics frame 0 has just updated, as in models/racformer.py:316-342."""
        T, B = len(radar_points), len(radar_points[0])
        if any(len(frame) != B for frame in radar_points):
            raise ValueError("RadarPillarEncoder: every frame needs one cloud per sample")
        if self.train_route():
            first = self._clouds_train(list(radar_points[0])).unsqueeze(1)
            if T == 1:
                return first
            rest = self._eval_frames([radar_points[t][b] for b in range(B) for t in range(1, T)])
            return torch.cat([first, rest.view(B, T - 1, *rest.shape[1:])], dim=1)
        out = self._clouds([radar_points[t][b] for b in range(B) for t in range(T)])
        return out.view(B, T, *out.shape[1:])


class _RadarTrainCore(torch.autograd.Function):
    """The branch's HIP training forward under autograd: apply(encoder, points, cloud_offsets, *encoder.train_params()) ->
    [n_clouds, 256, H, W].  The parameters are passed for autograd's bookkeeping and read from the modules.  The backward walks the
    stages last to first -- per ConvModule rac_bn_train_bwd, ``resnet.conv_wgrad``, ``resnet.conv_dgrad`` (its mask applies the ReLU
    of the layer in front, whose BatchNorm backward then takes the gradient as it is), then rac_pillar_train_bwd -- and runs a launch
    only where ``ctx.needs_input_grad`` asks for its result or for something in front of it.  Nothing is read back but the weight
    maxima of a pack whose weight changed.  The points get no gradient."""

    @staticmethod
    def forward(ctx, enc, points, cloud_offsets, *params):
        out, pfn_saved, layers = enc.train_forward_hip(points, cloud_offsets)
        ctx.enc = enc
        ctx.save_for_backward(*pfn_saved, *[t for layer in layers for t in layer])
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, gout):
        from . import resnet
        enc = ctx.enc
        pfn_saved, rest = ctx.saved_tensors[:8], ctx.saved_tensors[8:]
        layers = [rest[5 * i:5 * i + 5] for i in range(3)]
        flags = ctx.needs_input_grad[3:]
        grads = [None] * len(flags)
        wanted = [k for k in range(4) if any(flags[3 * k:3 * k + 3])]          # stage 0: the PFN layer; stage i + 1: ConvModule i
        if not wanted:
            return (None, None, None, *grads)
        first = wanted[0]
        g = gout.contiguous()
        for i in (2, 1, 0):
            x, z, y, mean, invstd = layers[i]
            nw, ng, nb = flags[3 * i + 3:3 * i + 6]
            front = first < i + 1
            bn = enc.radar_bev_conv[i].bn
            dgamma, dbeta, gz = bn_train_bwd(g, z, y if i == 2 else None, mean, invstd, bn.weight, need_dx=bool(nw or front))
            if nw:
                grads[3 * i + 3] = resnet.conv_wgrad(gz, x, 3, 1, bias=False)[0]
            grads[3 * i + 4], grads[3 * i + 5] = dgamma if ng else None, dbeta if nb else None
            if not front:
                return (None, None, None, *grads)
            # (the canvas needs no mask: the PFN backward takes its own ReLU decision from the saved features)
            g = resnet.conv_dgrad(gz, enc.train_packs(i, transposed=True), 3, 1, x.shape[2:], mask=x if i > 0 else None)
        dw, dgamma, dbeta = enc.radar_voxel_encoder.train_bwd(pfn_saved, g, need_dw=bool(flags[0]))
        grads[0], grads[1], grads[2] = dw, dgamma if flags[1] else None, dbeta if flags[2] else None
        return (None, None, None, *grads)
