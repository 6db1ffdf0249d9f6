"""CPU restatement of the Lift-Splat view transform (models/necks/view_transformer_racformer.py:112-295 of the reference) in plain
torch, float32 or float64: scaled coordinates, cells, the five tables with ascending ``ranks_depth`` inside a cell, the
channel-first output and -- through autograd -- the gradients.  Pinned to the reference by tests/golden/lss_view_small.npz
(tests/test_lss_view_ref.py); shares no code with racformer_amd/lss_view.py beyond the frustum construction it checks.

Point p = ((bn*D + d)*H + h)*W + w, pixel = bn*H*W + h*W + w, cell = ((b*Z + z)*Y + y)*X + x."""
import numpy as np
import torch


def img2lidar_f32(img_metas):
    """np.linalg.inv in the matrices' own dtype, then float32 (:139-147) -> [B*N, 4, 4]"""
    inv = np.asarray([[np.linalg.inv(m) for m in meta["lidar2img"]] for meta in img_metas]).astype(np.float32)
    return torch.from_numpy(inv.reshape(-1, 4, 4))


def lidar_points(img2lidar, depth_tab, v_tab, u_tab, dtype=torch.float32):
    """[B*N, D, H, W, 3]: M . (u*max(d,1e-5), v*max(d,1e-5), d, 1), first three components, in ``dtype`` (get_lidar_coor)."""
    d, v, u = depth_tab.to(dtype), v_tab.to(dtype), u_tab.to(dtype)
    D, H, W = d.numel(), v.numel(), u.numel()
    s = torch.maximum(d, torch.ones_like(d) * 1e-5).view(D, 1, 1)
    pts = torch.stack(((u.view(1, 1, W) * s).expand(D, H, W), (v.view(1, H, 1) * s).expand(D, H, W),
                       d.view(D, 1, 1).expand(D, H, W), torch.ones(D, H, W, dtype=dtype)), -1)          # [D,H,W,4]
    m = img2lidar.to(dtype)
    return torch.matmul(m.view(-1, 1, 1, 1, 4, 4), pts.view(1, D, H, W, 4, 1)).squeeze(-1)[..., :3]


def scaled_coords(img2lidar, depth_tab, v_tab, u_tab, lower, interval, dtype=torch.float32):
    """[B*N, D, H, W, 3]: (point - lower) / interval, a true division in ``dtype``."""
    xyz = lidar_points(img2lidar, depth_tab, v_tab, u_tab, dtype)
    return (xyz - torch.tensor(lower, dtype=dtype)) / torch.tensor(interval, dtype=dtype)


def cells_of(scaled, size, n_cams):
    """int64 [B*N*D*H*W]: truncation toward zero per axis (so (-1, 0) lands in cell 0 and is kept), -1 if dropped."""
    X, Y, Z = size
    idx = scaled.long()                                                     # trunc toward zero
    kept = ((idx[..., 0] >= 0) & (idx[..., 0] < X) & (idx[..., 1] >= 0) & (idx[..., 1] < Y)
            & (idx[..., 2] >= 0) & (idx[..., 2] < Z))
    b = (torch.arange(scaled.shape[0]) // n_cams).view(-1, 1, 1, 1)
    cell = ((b * Z + idx[..., 2]) * Y + idx[..., 1]) * X + idx[..., 0]
    return torch.where(kept, cell, torch.full_like(cell, -1)).reshape(-1)


def tables_of(cells, D, HW):
    """(ranks_bev, ranks_depth, ranks_feat, interval_starts, interval_lengths), int64: sorted by cell, ascending point index
    inside a cell (a stable sort of the kept points, which are in index order)."""
    kept = torch.nonzero(cells >= 0).flatten()
    order = torch.argsort(cells[kept], stable=True)
    rd = kept[order]
    rb = cells[rd]
    rf = (rd // (D * HW)) * HW + rd % HW
    if rb.numel() == 0:
        z = torch.zeros(0, dtype=torch.int64)
        return rb, rd, rf, z, z.clone()
    _, lengths = torch.unique_consecutive(rb, return_counts=True)
    return rb, rd, rf, torch.cumsum(lengths, 0) - lengths, lengths


def splat(depth_digit, tran_feat, cells, batch, size, dtype=torch.float32):
    """bev [B, Z*C, Y, X] (channel z*C + c) = sum over a cell's points, IN ASCENDING POINT ORDER, of
    softmax_D(logits)[point] * feat[pixel(point), :]; differentiable in both inputs."""
    X, Y, Z = size
    BN, D, H, W = depth_digit.shape
    C = tran_feat.shape[1]
    p = depth_digit.to(dtype).softmax(dim=1).reshape(-1)
    feat = tran_feat.to(dtype).permute(0, 2, 3, 1).reshape(BN * H * W, C)
    rb, rd, rf, _, _ = tables_of(cells, D, H * W)
    out = torch.zeros(batch * Z * Y * X, C, dtype=dtype)
    out = out.index_add(0, rb, p[rd].unsqueeze(1) * feat[rf])       # (a serial loop over the index on the CPU: sequential sums)
    return out.view(batch, Z, Y, X, C).permute(0, 1, 4, 2, 3).reshape(batch, Z * C, Y, X)


def view_transform(depth_digit, tran_feat, img2lidar, depth_tab, v_tab, u_tab, lower, interval, size, batch,
                   dtype=torch.float32, cells=None):
    """(bev, cells, scaled): the whole restatement; ``cells`` given: splat on those instead of the restatement's own."""
    scaled = scaled_coords(img2lidar, depth_tab, v_tab, u_tab, lower, interval, dtype)
    own = cells_of(scaled, size, img2lidar.shape[0] // batch)
    return splat(depth_digit, tran_feat, own if cells is None else cells, batch, size, dtype), own, scaled


def quirk_points(scaled, cells):
    """kept points with a scaled coordinate in (-1, 0) on some axis: kept only because .long() truncates toward zero"""
    neg = ((scaled > -1) & (scaled < 0)).any(-1).reshape(-1)
    return neg & (cells >= 0)


# ---------------------------------------------------------------------------------------------------------------- rigs
def grid_of(grid_config):
    """(lower, interval, size) per (x, y, z) through the reference's float32 tensors (create_grid_infos, :82-85)"""
    axes = [grid_config[k] for k in ("x", "y", "z")]
    lower = torch.Tensor([a[0] for a in axes])
    interval = torch.Tensor([a[2] for a in axes])
    size = torch.Tensor([(a[1] - a[0]) / a[2] for a in axes])
    return tuple(float(v) for v in lower), tuple(float(v) for v in interval), tuple(int(v) for v in size)


def frustum_axes(frustum):
    """(depth [D], v [H], u [W]) of a [D,H,W,3] frustum whose last dimension is (u, v, d)"""
    return frustum[:, 0, 0, 2].contiguous(), frustum[0, :, 0, 1].contiguous(), frustum[0, 0, :, 0].contiguous()


def golden_fixture(golden_dir, tag):
    """Fixture ``tag`` of tests/golden/lss_view_small.npz as a dict of tensors / plain values (no pickled objects)."""
    import os
    z = np.load(os.path.join(golden_dir, "lss_view_small.npz"), allow_pickle=False)
    fx = {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(tag + ":")}
    out = {k: (torch.from_numpy(v) if v.dtype.kind in "fi" and v.ndim else v) for k, v in fx.items()}
    out["grid_config"] = {a: [float(x) for x in fx["grid_" + a]] for a in ("x", "y", "z", "depth")}
    out["img_metas"] = [dict(lidar2img=[m for m in sample]) for sample in fx["lidar2img"]]
    out["input_size"] = tuple(int(v) for v in fx["input_size"])
    out["downsample"] = int(fx["downsample"])
    out["state_keys"] = [str(k) for k in fx["state_keys"]]
    return out
