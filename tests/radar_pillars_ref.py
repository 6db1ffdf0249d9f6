"""Independent restatement of the radar pillar branch (models/racformer.py:130-177 with mmcv 1.6.0's hard Voxelization, mmdet3d
1.0.0rc6's PillarFeatureNet / PointPillarsScatter and the three ConvModules of radar_bev_conv, :81-99) for the tests of
racformer_amd/radar_pillars.py.  It shares no code with that module: the voxelization is the plain sequential loop with a dict, in
numpy float32; the remaining stages are torch.nn.Linear / BatchNorm1d / Conv2d / BatchNorm2d modules in eval mode with the
BatchNorms UNFOLDED, in float32 or float64 (a folded float32 variant exists for the tolerance's basis only)."""
import numpy as np
import torch
import torch.nn as nn

F8 = dict(voxel_size=[0.8, 0.8, 8], point_cloud_range=[-51.2, -51.2, -5.0, 51.2, 51.2, 3.0], max_num_points=10, max_voxels=40000)
HAND = dict(voxel_size=[0.8, 0.8, 8], point_cloud_range=[-1.6, -1.6, -5, 1.6, 1.6, 3], max_num_points=2, max_voxels=3)
SMALL = dict(voxel_size=[0.8, 0.8, 8], point_cloud_range=[-6.4, -6.4, -5.0, 6.4, 6.4, 3.0], max_num_points=10, max_voxels=40000)


def grid_of(voxel_size, point_cloud_range):
    r, vs = np.asarray(point_cloud_range, np.float32), np.asarray(voxel_size, np.float32)
    return [int(v) for v in np.round((r[3:] - r[:3]) / vs)]


def cell_f32(value, lo, vs):
    """floor((p - lo) / vs) in IEEE float32: one subtraction, one correctly rounded division, floor"""
    return np.floor((np.float32(value) - np.float32(lo)) / np.float32(vs))


def cell_reciprocal_f32(value, lo, vs):
    """the form that is NOT allowed: multiply by the rounded reciprocal"""
    return np.floor((np.float32(value) - np.float32(lo)) * (np.float32(1) / np.float32(vs)))


def hard_voxelize(points, voxel_size, point_cloud_range, max_num_points, max_voxels):
    """points [n, C] (numpy float32) -> (voxels [M, P, C], coors [M, 3] = (z, y, x) int32, num_points [M] int32, kept): the
    sequential definition.  ``kept`` lists (point index, pillar, slot) for the tests that name points."""
    points = np.asarray(points, np.float32)
    grid = grid_of(voxel_size, point_cloud_range)
    table, voxels, coors, num, kept = {}, [], [], [], []
    for i in range(points.shape[0]):
        c = [cell_f32(points[i, j], point_cloud_range[j], voxel_size[j]) for j in range(3)]
        if not all(0 <= c[j] < grid[j] for j in range(3)):       # (a NaN fails the comparison and is skipped)
            continue
        cell = (int(c[2]), int(c[1]), int(c[0]))
        if cell not in table:
            if len(voxels) >= max_voxels:
                continue
            table[cell] = len(voxels)
            voxels.append(np.zeros((max_num_points, points.shape[1]), np.float32))
            coors.append(cell)
            num.append(0)
        v = table[cell]
        if num[v] < max_num_points:
            voxels[v][num[v]] = points[i]
            kept.append((i, v, num[v]))
            num[v] += 1
    M, C = len(voxels), points.shape[1]
    return (np.stack(voxels) if M else np.zeros((0, max_num_points, C), np.float32),
            np.asarray(coors, np.int32).reshape(M, 3), np.asarray(num, np.int32), kept)


def voxelize_batch(clouds, zero_z=False, **cfg):
    """The reference's radar_voxelize: per cloud, concatenated, the sample index prepended -> torch (voxels, coors [M, 4], num)."""
    vs, cs, ns = [], [], []
    for b, p in enumerate(clouds):
        p = (p.numpy() if torch.is_tensor(p) else np.asarray(p)).astype(np.float32)         # (a copy)
        if zero_z:
            p[:, 2] = 0
        v, c, n, _ = hard_voxelize(p, **cfg)
        vs.append(v)
        cs.append(np.concatenate([np.full((c.shape[0], 1), b, np.int32), c], axis=1))
        ns.append(n)
    return torch.from_numpy(np.concatenate(vs)), torch.from_numpy(np.concatenate(cs)), torch.from_numpy(np.concatenate(ns))


# ------------------------------------------------------------------------------------------------ weights
def make_state_dict(seed, in_channels=7, embed_dims=256):
    """A seeded state dict under the detector's key names, with running statistics away from (0, 1) so that the BatchNorms do
    something, and positive as well as negative shifts."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)        # noqa: E731
    sd = {}

    def bn(prefix, c):
        sd[prefix + "weight"] = 1.0 + 0.3 * rn(c)
        sd[prefix + "bias"] = 0.2 * rn(c)
        sd[prefix + "running_mean"] = 0.3 * rn(c)
        sd[prefix + "running_var"] = 0.5 + torch.rand(c, generator=g)
        sd[prefix + "num_batches_tracked"] = torch.tensor(7)

    sd["radar_voxel_encoder.pfn_layers.0.linear.weight"] = rn(64, in_channels + 6) * 0.3
    bn("radar_voxel_encoder.pfn_layers.0.norm.", 64)
    for i, (ci, co) in enumerate([(64, 64), (64, 64), (64, embed_dims)]):
        sd[f"radar_bev_conv.{i}.conv.weight"] = rn(co, ci, 3, 3) / 24.0
        bn(f"radar_bev_conv.{i}.bn.", co)
    return sd


STATE_DICT_KEYS = sorted(make_state_dict(0).keys())


class Stages:
    """The nn modules of the branch in one dtype, eval mode, loaded from a state dict."""

    def __init__(self, sd, dtype, voxel_size, point_cloud_range, **_):
        k = "radar_voxel_encoder.pfn_layers.0."
        w = sd[k + "linear.weight"]
        self.dtype = dtype
        self.linear = nn.Linear(w.shape[1], w.shape[0], bias=False)
        self.norm = nn.BatchNorm1d(w.shape[0], eps=1e-3)
        self.linear.load_state_dict({"weight": w})
        self.norm.load_state_dict({n: sd[k + "norm." + n] for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")})
        self.convs = []
        for i in range(3):
            cw = sd[f"radar_bev_conv.{i}.conv.weight"]
            conv, bn = nn.Conv2d(cw.shape[1], cw.shape[0], 3, padding=1, bias=False), nn.BatchNorm2d(cw.shape[0], eps=1e-5)
            conv.load_state_dict({"weight": cw})
            bn.load_state_dict({n: sd[f"radar_bev_conv.{i}.bn." + n] for n in ("weight", "bias", "running_mean", "running_var",
                                                                                 "num_batches_tracked")})
            self.convs.append((conv.to(dtype).eval(), bn.to(dtype).eval()))
        self.linear, self.norm = self.linear.to(dtype).eval(), self.norm.to(dtype).eval()
        self.vs, self.rng = [float(v) for v in voxel_size], [float(v) for v in point_cloud_range]
        self.grid = grid_of(voxel_size, point_cloud_range)

    def decorate(self, voxels, coors, num):
        """[M, P, C] -> the masked [M, P, C + 6] features (PillarFeatureNet.forward, legacy=False)"""
        v = voxels.to(self.dtype)
        mean = v[:, :, :3].sum(dim=1, keepdim=True) / num.to(self.dtype).view(-1, 1, 1)
        f_cluster = v[:, :, :3] - mean
        f_center = torch.zeros_like(f_cluster)
        for j, col in enumerate((3, 2, 1)):               # x <- c_x (coors column 3), y <- c_y, z <- c_z
            f_center[:, :, j] = v[:, :, j] - (coors[:, col].to(self.dtype).unsqueeze(1) * self.vs[j] + (self.vs[j] / 2 + self.rng[j]))
        f = torch.cat([v, f_cluster, f_center], dim=-1)
        mask = (torch.arange(v.shape[1]).view(1, -1) < num.view(-1, 1)).to(self.dtype).unsqueeze(-1)
        return f * mask

    @torch.no_grad()
    def pillar_features(self, voxels, coors, num, folded=False):
        """-> [M, 64]: Linear, BatchNorm1d (running statistics), ReLU, max over ALL rows (the padded ones included)"""
        f = self.decorate(voxels, coors, num)
        if f.shape[0] == 0:
            return f.new_zeros(0, self.linear.out_features)
        if folded:
            g = self.norm.weight / torch.sqrt(self.norm.running_var + self.norm.eps)
            x = f @ (self.linear.weight * g.view(-1, 1)).t() + (self.norm.bias - self.norm.running_mean * g)
        else:
            x = self.norm(self.linear(f).transpose(1, 2)).transpose(1, 2)
        return torch.relu(x).max(dim=1)[0]

    def scatter(self, feats, coors, batch):
        canvas = feats.new_zeros(batch, feats.shape[1], self.grid[1], self.grid[0])
        for i in range(feats.shape[0]):
            canvas[int(coors[i, 0]), :, int(coors[i, 2]), int(coors[i, 3])] = feats[i]
        return canvas

    def canvas(self, voxels, coors, num, batch, folded=False):
        return self.scatter(self.pillar_features(voxels, coors, num, folded), coors, batch)

    @torch.no_grad()
    def conv_layer(self, i, x):
        conv, bn = self.convs[i]
        return torch.relu(bn(conv(x.to(self.dtype))))

    def stack_stages(self, canvas):
        """[canvas, after layer 0, 1, 2]"""
        out = [canvas.to(self.dtype)]
        for i in range(3):
            out.append(self.conv_layer(i, out[-1]))
        return out

    def folded_conv_l1(self, i):
        """max-row L1 norm of layer i's convolution with its BatchNorm folded in (float64): the layer's gain in the max norm"""
        conv, bn = self.convs[i]
        g = (bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)).abs()
        return float((conv.weight.detach().double().abs().sum(dim=(1, 2, 3)) * g.detach()).max())


def canvas_e_ref(sd, cfg, voxels, coors, num, batch):
    """(float64 canvas, E_ref): E_ref = max(|f32 unfolded - f64|, |f32 folded - f64|, |f32 folded - f32 unfolded|)"""
    s64, s32 = Stages(sd, torch.float64, **cfg), Stages(sd, torch.float32, **cfg)
    c64 = s64.canvas(voxels, coors, num, batch)
    a, b = s32.canvas(voxels, coors, num, batch).double(), s32.canvas(voxels, coors, num, batch, folded=True).double()
    return c64, max(float((a - c64).abs().max()), float((b - c64).abs().max()), float((b - a).abs().max()))


def forward(sd, cfg, frames, dtype):
    """frames: list over T of list over B of clouds -> ([B, T, 256, H, W] by torch.stack(..., dim=1) of the per-frame results,
    per-frame list of stage lists); z treated as 0."""
    st = Stages(sd, dtype, **cfg)
    per_frame, stages = [], []
    for clouds in frames:
        v, c, n = voxelize_batch(clouds, zero_z=True, **cfg)
        s = st.stack_stages(st.canvas(v, c, n, len(clouds)))
        stages.append(s)
        per_frame.append(s[-1])
    return torch.stack(per_frame, dim=1), stages
