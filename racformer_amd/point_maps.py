"""Point clouds to per-view maps: the ``radar_depth`` / ``radar_rcs`` maps of the reference's ``RadarPointToMultiViewDepth`` and the
``gt_depth`` map of its ``PointToMultiViewDepth`` (loaders/pipelines/loading.py:470-600), made from the packed clouds of the radar
pillar ABI (``radar_pillars.pack_clouds``) and a table of view matrices.  On device tensors: ``rac_point_maps_radar_fwd`` /
``rac_point_maps_lidar_fwd`` (csrc/point_maps.hip) -- nothing read back, capturable, the same bits every run.  On CPU tensors: the
restatement below, which is also what the kernels are tested against, bit for bit.

The rules, for one cloud and one view with ``M`` the float32 ``lidar2img``:

1. ``p_i = x M[i,0] + y M[i,1] + z M[i,2] + M[i,3]``, float32, left to right, every operation rounded once; ``u = p_0 / p_2``,
   ``v = p_1 / p_2``, ``d = p_2``; ``cx = rint(u / ds)``, ``cy = rint(v / ds)`` (half to even).  The map is ``H // ds x W // ds``.
2. kept: ``0 <= cx < wm``, ``0 <= cy < hm``, ``lo <= d < hi`` (NaN, inf and ``p_2 = 0`` fail).
3. key ``k = (cx + cy wm) + d / 100`` in float32; a pixel's winner is the kept point with the smallest ``(k, index)`` -- what a stable
   sort gives where the reference's ``argsort`` leaves ties unspecified.
4. lidar: ``out[cy, cx] = d`` of the pixel's winner, 0 elsewhere.
5. radar: the reference writes whole columns, the last write wins: a column holds the value of its pixel winner with the largest
   ``cy``.  ``radar_rcs`` gets ``points[s, rcs_col]`` with ``s`` the winner's position among the kept points in input order, not the
   winner's own RCS: the reference filters ``coor`` and ``depth`` by the kept mask but not ``RCS``.  Kept as it is.
6. frame ``t``'s cloud goes with ``lidar2img[t N : (t + 1) N]``; map index ``cloud * N + view``.

The device route refuses what the restatement accepts but the key no longer orders as the reference's sort does: more than 2^18
pixels, ``hi > 99``, ``lo <= 0``, 2^20 points or more, more than 4096 rows (``LIMITS``)."""
import ctypes

import numpy as np
import torch

from . import _lib
from .radar_pillars import pack_clouds  # noqa: F401  (the one packing both consumers of the radar clouds use)

RCS_COLUMN = 3
LIMITS = dict(pixels=1 << 18, hi=99.0, points=1 << 20, rows=4096)


# ------------------------------------------------------------------------------------------------ the view table
def view_table(lidar2img, device=None):
    """4x4 (or 3x4) matrices -- a list of arrays / tensors or one array [..., >= 3, 4] -- as the kernels' float32 table [n, 12]: rows
    0..2 of each, cast to float32 as the reference casts them.  One small host tensor, copied once."""
    if isinstance(lidar2img, torch.Tensor):
        m = lidar2img.detach().to("cpu").numpy()
    else:
        m = np.stack([np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x) for x in lidar2img]) if len(lidar2img) else \
            np.zeros((0, 4, 4), np.float32)
    if m.ndim == 2 and m.shape[1] == 12:
        m = m.reshape(-1, 3, 4)
    if m.ndim < 3 or m.shape[-1] != 4 or m.shape[-2] < 3:
        raise ValueError(f"view_table: matrices of shape [..., >= 3, 4] expected, got {m.shape}")
    table = torch.from_numpy(np.ascontiguousarray(m.reshape(-1, *m.shape[-2:])[:, :3, :].astype(np.float32).reshape(-1, 12)))
    return table if device is None else table.to(device)


def meta_view_table(img_metas, num_views, frames=None, device=None):
    """The table for a batch of metas: per sample ``img_metas[b]['lidar2img'][: frames * num_views]`` (all of them when ``frames`` is
    None), samples back to back -- the order of clouds ``[b][t]`` packed sample-major."""
    mats = []
    for meta in img_metas:
        l2i = list(meta["lidar2img"])
        count = len(l2i) if frames is None else frames * num_views
        if count > len(l2i) or count % num_views:
            raise ValueError(f"meta_view_table: {len(l2i)} matrices, {count} needed in groups of {num_views}")
        mats += l2i[:count]
    return view_table(mats, device)


# ------------------------------------------------------------------------------------------------ arguments
def _geometry(points, cloud_offsets, mats, hw, grid_config, downsample, pad_hw, what):
    if points.dim() != 2 or points.dtype != torch.float32 or points.shape[1] < 3:
        raise TypeError(f"{what}: float32 points [n, >= 3] expected")
    if cloud_offsets.dtype != torch.int32 or cloud_offsets.dim() != 1 or cloud_offsets.numel() < 2:
        raise TypeError(f"{what}: int32 cloud_offsets [n_clouds + 1] expected")
    if not isinstance(mats, torch.Tensor) or mats.dim() != 2 or mats.shape[1] != 12:
        mats = view_table(mats)
    mats = mats.to(points.device, torch.float32).contiguous()
    n_clouds = cloud_offsets.numel() - 1
    if mats.shape[0] == 0 or mats.shape[0] % n_clouds:
        raise ValueError(f"{what}: {mats.shape[0]} view matrices for {n_clouds} clouds")
    ds = int(downsample)
    if ds < 1:
        raise ValueError(f"{what}: downsample={downsample} (at least 1)")
    H, W = int(hw[0]), int(hw[1])
    hm, wm = H // ds, W // ds
    if hm < 1 or wm < 1:
        raise ValueError(f"{what}: a {H} x {W} image has no map at downsample={ds}")
    hp, wp = (hm, wm) if pad_hw is None else (int(pad_hw[0]), int(pad_hw[1]))
    if hp < hm or wp < wm:
        raise ValueError(f"{what}: pad_hw {(hp, wp)} is smaller than the map {(hm, wm)}")
    lo, hi = float(grid_config["depth"][0]), float(grid_config["depth"][1])
    return mats, n_clouds, mats.shape[0] // n_clouds, (H, W, hm, wm, hp, wp, ds), (lo, hi)


# ------------------------------------------------------------------------------------------------ the restatement
def _project(p, M, hm, wm, ds, lo, hi):
    """Rules 1-3 for one cloud [n, C] and one view M [12] -> (kept [n] bool, cx, cy int64, d, k float32), elementwise in the fixed order."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    row = [x * M[4 * i] + y * M[4 * i + 1] + z * M[4 * i + 2] + M[4 * i + 3] for i in range(3)]
    d = row[2]
    f = torch.tensor(float(ds), dtype=torch.float32, device=p.device)
    fx, fy = torch.round(row[0] / d / f), torch.round(row[1] / d / f)
    kept = (fx >= 0) & (fx < wm) & (fy >= 0) & (fy < hm) & (d < hi) & (d >= lo)
    k = (fx + fy * float(wm)) + d / torch.tensor(100.0, dtype=torch.float32, device=p.device)
    return kept, fx, fy, d, k


def _pixel_winners(kept, fx, fy, k, wm):
    """-> (s, cx, cy): per occupied pixel the winner's position among the kept points and its pixel, pixels ascending."""
    s_all = torch.nonzero(kept).flatten()           # kept points in input order: position s -> index
    cx, cy, kk = fx[s_all].long(), fy[s_all].long(), k[s_all]
    by_key = torch.sort(kk, stable=True).indices                       # the smallest (k, index) first ...
    pixel = (cy * wm + cx)[by_key]
    by_pixel = torch.sort(pixel, stable=True).indices                  # ... inside every pixel
    order, pixel = by_key[by_pixel], pixel[by_pixel]
    first = torch.ones_like(pixel, dtype=torch.bool)
    first[1:] = pixel[1:] != pixel[:-1]
    s = order[first]
    return s, s_all, cx[s], cy[s]


def _clouds(points, cloud_offsets):
    off = cloud_offsets.detach().cpu().tolist()
    return [(off[c], points[off[c]:off[c + 1]]) for c in range(len(off) - 1)]


def radar_maps_torch(points, cloud_offsets, lidar2img, hw, grid_config, downsample=1, pad_hw=None, rcs_col=RCS_COLUMN, winners=None):
    """Rules 1-6 in torch on the points' device -> (radar_depth, radar_rcs) [n_clouds * N, Hp, Wp] float32.  ``winners``: a list that
    receives per map an int64 [wm] of each column's winning point (its index in the packed ``points``; -1 for an empty column)."""
    mats, n_clouds, N, (H, W, hm, wm, hp, wp, ds), (lo, hi) = _geometry(points, cloud_offsets, lidar2img, hw, grid_config, downsample,
                                                                          pad_hw, "radar_maps_torch")
    if not 0 <= rcs_col < points.shape[1]:
        raise ValueError(f"radar_maps_torch: RCS column {rcs_col} outside [0, {points.shape[1]})")
    depth = points.new_zeros(n_clouds * N, hp, wp)
    rcs = points.new_zeros(n_clouds * N, hp, wp)
    for c, (start, p) in enumerate(_clouds(points.detach(), cloud_offsets)):
        for v in range(N):
            m = c * N + v
            kept, fx, fy, d, k = _project(p, mats[m], hm, wm, ds, lo, hi)
            s, s_all, cx, cy = _pixel_winners(kept, fx, fy, k, wm)
            if winners is not None:
                winners.append(torch.full((wm,), -1, dtype=torch.long, device=p.device))
            if s.numel() == 0:
                continue
            by_col = torch.sort(cx, stable=True).indices            # pixels ascend, so inside a column cy ascends: the last one wins
            col = cx[by_col]
            last = torch.ones_like(col, dtype=torch.bool)
            last[:-1] = col[1:] != col[:-1]
            w = s[by_col][last]
            row = points.new_zeros(2, wp)
            row[0, col[last]] = d[s_all[w]]
            row[1, col[last]] = p[w, rcs_col]                       # (rule 5: the point at the winner's position among the kept ones)
            depth[m, :hm], rcs[m, :hm] = row[0], row[1]             # the whole column
            if winners is not None:
                winners[-1][col[last]] = s_all[w] + start
    return depth, rcs


def lidar_depth_map_torch(points, cloud_offsets, lidar2img, hw, grid_config, downsample=1, pad_hw=None, winners=None):
    """Rules 1-4 and 6 in torch on the points' device -> gt_depth [n_clouds * N, Hp, Wp] float32.  ``winners``: a list that receives
    per map an int64 [hm, wm] of each pixel's winning point (its index in the packed ``points``; -1 for an empty pixel)."""
    mats, n_clouds, N, (H, W, hm, wm, hp, wp, ds), (lo, hi) = _geometry(points, cloud_offsets, lidar2img, hw, grid_config, downsample,
                                                                          pad_hw, "lidar_depth_map_torch")
    out = points.new_zeros(n_clouds * N, hp, wp)
    for c, (start, p) in enumerate(_clouds(points.detach(), cloud_offsets)):
        for v in range(N):
            m = c * N + v
            kept, fx, fy, d, k = _project(p, mats[m], hm, wm, ds, lo, hi)
            s, s_all, cx, cy = _pixel_winners(kept, fx, fy, k, wm)
            out[m, cy, cx] = d[s_all[s]]
            if winners is not None:
                winners.append(torch.full((hm, wm), -1, dtype=torch.long, device=p.device))
                winners[-1][cy, cx] = s_all[s] + start
    return out


# ------------------------------------------------------------------------------------------------ the device route
def radar_scratch_words(n_maps, wm):
    return 2 * n_maps * wm


def lidar_scratch_words(n_maps, hm, wm):
    return n_maps * hm * wm


def _device_args(points, cloud_offsets, mats, what):
    _lib.require_gpu(points, cloud_offsets, mats, what=what)
    if cloud_offsets.device != points.device:
        raise ValueError(f"{what}: points and cloud_offsets on different devices")


def radar_maps_fwd(points, cloud_offsets, mats, hw, lo, hi, downsample=1, pad_hw=None, rcs_col=RCS_COLUMN, depth=None, rcs=None,
                   scratch=None, want=(True, True)):
    """``rac_point_maps_radar_fwd`` on given buffers (``depth`` / ``rcs`` [n_maps, Hp, Wp] float32, ``scratch`` int64
    [>= radar_scratch_words]; allocated when None; ``want``: which of the two maps to make when they are allocated here)."""
    _device_args(points, cloud_offsets, mats, "radar_maps_fwd")
    ds = int(downsample)
    H, W = int(hw[0]), int(hw[1])
    hm, wm = H // max(ds, 1), W // max(ds, 1)
    hp, wp = (hm, wm) if pad_hw is None else (int(pad_hw[0]), int(pad_hw[1]))
    n_clouds, n_maps = cloud_offsets.numel() - 1, mats.shape[0]
    if depth is None and want[0]:
        depth = torch.empty(n_maps, hp, wp, dtype=torch.float32, device=points.device)
    if rcs is None and want[1]:
        rcs = torch.empty(n_maps, hp, wp, dtype=torch.float32, device=points.device)
    for o in (depth, rcs):
        if o is not None and (o.dtype != torch.float32 or not o.is_contiguous() or o.numel() != n_maps * hp * wp or o.device != points.device):
            raise ValueError(f"radar_maps_fwd: a contiguous float32 output of {n_maps} x {hp} x {wp} elements on the points' device expected")
    if scratch is None:
        scratch = torch.empty(max(radar_scratch_words(n_maps, wm), 1), dtype=torch.int64, device=points.device)
    null = ctypes.c_void_p(None)
    rc = _lib.lib().rac_point_maps_radar_fwd(_lib.ptr(points), _lib.ptr(cloud_offsets), _lib.ptr(mats), _lib.ptr(depth) if depth is not None else null,
                                             _lib.ptr(rcs) if rcs is not None else null, _lib.ptr(scratch), scratch.numel(), points.shape[0],
                                             n_clouds, n_maps // n_clouds, points.shape[1], int(rcs_col), H, W, hp, wp, ds, float(lo), float(hi),
                                             _lib.stream_ptr())
    _lib.check(rc, "rac_point_maps_radar_fwd")
    return depth, rcs


def lidar_depth_map_fwd(points, cloud_offsets, mats, hw, lo, hi, downsample=1, pad_hw=None, out=None, scratch=None):
    """``rac_point_maps_lidar_fwd`` on given buffers (``out`` [n_maps, Hp, Wp] float32, ``scratch`` int64 [>= lidar_scratch_words])."""
    _device_args(points, cloud_offsets, mats, "lidar_depth_map_fwd")
    ds = int(downsample)
    H, W = int(hw[0]), int(hw[1])
    hm, wm = H // max(ds, 1), W // max(ds, 1)
    hp, wp = (hm, wm) if pad_hw is None else (int(pad_hw[0]), int(pad_hw[1]))
    n_clouds, n_maps = cloud_offsets.numel() - 1, mats.shape[0]
    if out is None:
        out = torch.empty(n_maps, hp, wp, dtype=torch.float32, device=points.device)
    elif out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n_maps * hp * wp or out.device != points.device:
        raise ValueError(f"lidar_depth_map_fwd: a contiguous float32 output of {n_maps} x {hp} x {wp} elements on the points' device expected")
    if scratch is None:
        scratch = torch.empty(max(lidar_scratch_words(n_maps, hm, wm), 1), dtype=torch.int64, device=points.device)
    rc = _lib.lib().rac_point_maps_lidar_fwd(_lib.ptr(points), _lib.ptr(cloud_offsets), _lib.ptr(mats), _lib.ptr(out), _lib.ptr(scratch),
                                             scratch.numel(), points.shape[0], n_clouds, n_maps // n_clouds, points.shape[1], H, W, hp, wp, ds,
                                             float(lo), float(hi), _lib.stream_ptr())
    _lib.check(rc, "rac_point_maps_lidar_fwd")
    return out


# ------------------------------------------------------------------------------------------------ the public pair
def radar_maps(points, cloud_offsets, lidar2img, hw, grid_config, downsample=1, pad_hw=None, rcs_col=RCS_COLUMN):
    """Packed radar clouds -> (radar_depth, radar_rcs) [n_clouds * N, Hp, Wp].  ``points`` [n, C] float32 and ``cloud_offsets`` int32
    [n_clouds + 1] from ``pack_clouds``; ``lidar2img``: ``view_table`` / ``meta_view_table``'s table [n_clouds * N, 12] or matrices it
    accepts; ``hw`` the image size, the map is ``H // downsample x W // downsample``; ``grid_config['depth'][:2]`` the kept range;
    ``pad_hw`` >= the map (pads are +0.0).  Device tensors: the HIP kernels; CPU tensors: ``radar_maps_torch``."""
    if not points.is_cuda:
        return radar_maps_torch(points, cloud_offsets, lidar2img, hw, grid_config, downsample, pad_hw, rcs_col)
    mats, _, _, (H, W, hm, wm, hp, wp, ds), (lo, hi) = _geometry(points, cloud_offsets, lidar2img, hw, grid_config, downsample, pad_hw,
                                                                   "radar_maps")
    return radar_maps_fwd(points.detach().contiguous(), cloud_offsets.contiguous(), mats, (H, W), lo, hi, ds, (hp, wp), rcs_col)


def lidar_depth_map(points, cloud_offsets, lidar2img, hw, grid_config, downsample=1, pad_hw=None):
    """Packed lidar clouds -> gt_depth [n_clouds * N, Hp, Wp]; arguments as ``radar_maps``."""
    if not points.is_cuda:
        return lidar_depth_map_torch(points, cloud_offsets, lidar2img, hw, grid_config, downsample, pad_hw)
    mats, _, _, (H, W, hm, wm, hp, wp, ds), (lo, hi) = _geometry(points, cloud_offsets, lidar2img, hw, grid_config, downsample, pad_hw,
                                                                   "lidar_depth_map")
    return lidar_depth_map_fwd(points.detach().contiguous(), cloud_offsets.contiguous(), mats, (H, W), lo, hi, ds, (hp, wp))
