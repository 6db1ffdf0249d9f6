"""oracle/restate.py -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

CPU restatement (plain torch-CPU / numpy, functional, weights read from a ``state_dict`` with
the reference's key names) of RaCFormer's query-decoder hot path.  It is the parity checker for
the HIP path: only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s ``cpu_baseline``
leg import it.  Nothing under ``racformer_amd/`` imports, calls or falls back to it.

Parity status: PINNED.  Every function below is checked in ``tests/test_oracle_vs_golden.py``
against fixtures produced by running the reference's own files on CPU in the build container
(``tests/golden/gen_golden.py``): op level (geometry, msmv, sampling_4d, MSDA), per-stage
outputs of decoder layer 0 / 5, and the full 6-layer decoder at reduced and at f8 shapes.
``head_forward`` / ``head_init_query`` / ``nms_free_decode`` (``models/racformer_head.py:51-134,488-507``,
``models/bbox/coders/nms_free_coder.py:37-88``) are pinned the same way since round 2: the two files load in the
build container once the mmdet / mmdet3d base classes they subclass are stubbed as plumbing
(``tests/golden/ref_loader.py``), fixtures ``decode_cases.npz``, ``head_small6.npz``, ``head_f8.npz``.
One thing the reference leaves open is pinned as such: the ORDER of exactly tied scores in ``Tensor.topk`` (and which
members of a tie group that straddles rank K are returned) is implementation-defined in torch -- tests accept any
member of the tie group there and exact positions everywhere else (``tests/parity.py::decode_parity``).

Each function cites the reference file:line it follows (paths relative to the reference root).
"""
import ctypes
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

_HERE = os.path.dirname(os.path.abspath(__file__))
_TWO_PI = 2 * math.pi


# =============================================================================== geometry
def decode_bbox(b, pc_range):
    """models/bbox/utils.py:66-80"""
    xyz = b[..., 0:3].clone()
    wlh = b[..., 3:6].exp()
    rot = torch.atan2(b[..., 6:7], b[..., 7:8])
    xyz[..., 0] = xyz[..., 0] * (pc_range[3] - pc_range[0]) + pc_range[0]
    xyz[..., 1] = xyz[..., 1] * (pc_range[4] - pc_range[1]) + pc_range[1]
    xyz[..., 2] = xyz[..., 2] * (pc_range[5] - pc_range[2]) + pc_range[2]
    tail = [b[..., 8:10]] if b.shape[-1] > 8 else []
    return torch.cat([xyz, wlh, rot] + tail, dim=-1)


def denormalize_bbox(nb):
    """models/bbox/utils.py:26-46  (input order cx,cy,w,l,cz,h,sin,cos,vx,vy)"""
    rot = torch.atan2(nb[..., 6:7], nb[..., 7:8])
    parts = [nb[..., 0:1], nb[..., 1:2], nb[..., 4:5], nb[..., 2:3].exp(), nb[..., 3:4].exp(),
             nb[..., 5:6].exp(), rot]
    if nb.shape[-1] > 8:
        parts += [nb[..., 8:9], nb[..., 9:10]]
    return torch.cat(parts, dim=-1)


def theta_d2xy(t, map_size=102.4, r=65.0):
    """models/bbox/utils.py:82-90: polar (theta in turns, d in units of r) -> normalised xy, clamped."""
    center = map_size / 2
    ang = t[..., 0:1] * _TWO_PI
    x = (center + t[..., 1:2] * r * torch.cos(ang)) / map_size
    y = (center + t[..., 1:2] * r * torch.sin(ang)) / map_size
    xy = torch.clamp(torch.cat([x, y], dim=-1), min=0, max=1)
    return torch.cat([xy, t[..., 2:]], dim=-1)


def xy2theta_d(p, map_size=102.4, r=65.0):
    """models/bbox/utils.py:93-100 (norm=True branch)"""
    center = map_size / 2
    dx = p[..., 0:1] * map_size - center
    dy = p[..., 1:2] * map_size - center
    dist = torch.sqrt(dx ** 2 + dy ** 2) / r
    theta = torch.atan2(dy, dx)
    theta = ((theta + _TWO_PI) % _TWO_PI) / _TWO_PI
    return torch.cat([theta, dist, p[..., 2:]], dim=-1)


def inverse_sigmoid(x, eps=1e-5):
    """models/utils.py:86-101"""
    x = x.clamp(min=0, max=1)
    return torch.log(x.clamp(min=eps) / (1 - x).clamp(min=eps))


def rotate_z(points, ang):
    """models/utils.py:48-83 (VERSION 'v1.0.0' branch): points [...,P,3], ang [...,1];
    x' = x c - y s ; y' = x s + y c."""
    c = torch.cos(ang)[..., None, :]     # [...,1,1]
    s = torch.sin(ang)[..., None, :]
    x, y, z = points[..., 0:1], points[..., 1:2], points[..., 2:3]
    return torch.cat([x * c - y * s, x * s + y * c, z], dim=-1)


def make_sample_points(query_bbox, offset, pc_range):
    """models/sparsebev_sampling.py:8-25"""
    d = decode_bbox(query_bbox, pc_range)
    xyz, wlh, ang = d[..., 0:3], d[..., 3:6], d[..., 6:7]
    delta = rotate_z(wlh[:, :, None, :] * offset[..., 0:3], ang)
    return xyz[:, :, None, :] + delta


# =============================================================================== gathers
_CLIB = None


def _clib():
    """ctypes handle of the C restatement (oracle/gather_ref.c), built by oracle/Makefile."""
    global _CLIB
    if _CLIB is None:
        path = os.path.join(_HERE, "libgather_ref.so")
        if not os.path.exists(path):
            return None
        lib = ctypes.CDLL(path)
        for fn in ("oracle_msmv_fwd", "oracle_msda_fwd", "oracle_msmv_fwd_f64", "oracle_msda_fwd_f64"):
            getattr(lib, fn).restype = ctypes.c_int
        _CLIB = lib
    return _CLIB


def _round_half_away(x):
    """round half away from zero, as C ``round`` / ``roundf`` (the reference's and the kernels' view pick,
    msmv_sampling_forward.cu:110); ``torch.round`` rounds half to even."""
    t = torch.trunc(x)
    return torch.where((x - t).abs() >= 0.5, t + torch.sign(x), t)   # x - trunc(x) is exact: no tie is made by rounding


def _coord(x, scale, shift, f32_coords):
    """``x * scale - shift``: the sampling coordinate of a normalised location.  With ``f32_coords`` and a wider
    input the value is formed in float32, as the kernels and the reference form it (one rounding per operation), and
    then promoted; the derivative stays ``scale`` in the input's precision.  A float64 reference then picks the same
    taps, guard and view as the kernel even where a float32 product rounds onto an integer."""
    y = x * scale - shift if shift else x * scale
    if f32_coords and x.dtype != torch.float32:
        y32 = x.detach().float() * scale
        if shift:
            y32 = y32 - shift
        y = y + (y32.to(y.dtype) - y.detach())
    return y


def _bilinear_taps(fmap, h_im, w_im):
    """fmap [H,W,C] (any leading index handled by caller); h_im,w_im [K] float32.
    4-tap bilinear with per-tap bounds checks (msmv_sampling_forward.cu:27-73)."""
    H, W, _ = fmap.shape
    h_low = torch.floor(h_im)
    w_low = torch.floor(w_im)
    lh, lw = h_im - h_low, w_im - w_low
    hh, hw = 1 - lh, 1 - lw
    h_low, w_low = h_low.long(), w_low.long()
    h_high, w_high = h_low + 1, w_low + 1

    def tap(hi, wi):
        ok = (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
        v = fmap[hi.clamp(0, H - 1), wi.clamp(0, W - 1)]
        return v * ok[:, None].to(v.dtype)

    return ((hh * hw)[:, None] * tap(h_low, w_low) + (hh * lw)[:, None] * tap(h_low, w_high)
            + (lh * hw)[:, None] * tap(h_high, w_low) + (lh * lw)[:, None] * tap(h_high, w_high))


def msmv_gather_torch(feats_cl, loc, w, f32_coords=False):
    """Pure-torch kernel-semantics msmv (small cases).  feats_cl[l]: [S,N,H,W,C]; loc [S,Q,P,3];
    w [S,Q,P,L] -> [S,Q,C,P], in the operands' dtype.  Follows msmv_sampling_forward.cu:105-162.
    ``f32_coords``: see ``_coord``."""
    S, N = feats_cl[0].shape[:2]
    C = feats_cl[0].shape[-1]
    _, Q, P, _ = loc.shape
    view = _round_half_away(_coord(loc[..., 2].detach(), N - 1, 0, f32_coords)).long().reshape(-1)
    sidx = torch.arange(S)[:, None, None].expand(S, Q, P).reshape(-1)
    u, v = loc[..., 0].reshape(-1), loc[..., 1].reshape(-1)
    out = torch.zeros(S * Q * P, C, dtype=torch.promote_types(feats_cl[0].dtype, loc.dtype))
    for l, f in enumerate(feats_cl):
        H, W = f.shape[2:4]
        h_im, w_im = _coord(v, H - 1, 0, f32_coords), _coord(u, W - 1, 0, f32_coords)
        guard = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
        flat = f.reshape(S * N, H, W, C)
        base = sidx * N + view
        # emulate per-map indexing by folding the map index into the row index
        big = flat.reshape(S * N * H, W, C)
        Hs = S * N * H

        def tap(hi, wi):
            ok = (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
            row = (base * H + hi.clamp(0, H - 1)).clamp(0, Hs - 1)
            return big[row, wi.clamp(0, W - 1)] * ok[:, None].float()

        h_low, w_low = torch.floor(h_im), torch.floor(w_im)
        lh, lw = h_im - h_low, w_im - w_low
        hh, hw = 1 - lh, 1 - lw
        hl, wl = h_low.long(), w_low.long()
        val = ((hh * hw)[:, None] * tap(hl, wl) + (hh * lw)[:, None] * tap(hl, wl + 1)
               + (lh * hw)[:, None] * tap(hl + 1, wl) + (lh * lw)[:, None] * tap(hl + 1, wl + 1))
        out = out + val * (guard.float() * w[..., l].reshape(-1))[:, None]
    return out.reshape(S, Q, P, C).permute(0, 1, 3, 2).contiguous()


def msmv_gather(feats_cl, loc, w, force_torch=False):
    """msmv op, kernel semantics, reference output layout [S,Q,C,P] (wrapper.py:145-153)."""
    lib = None if force_torch else _clib()
    if lib is None:
        return msmv_gather_torch(feats_cl, loc, w)
    # float32: the checker (the reference's arithmetic type).  float64 operands select the `_f64` instance of the same C text:
    # the arbiter of tools/fp64_arbiter.py.
    dt = torch.float64 if feats_cl[0].dtype == torch.float64 else torch.float32
    feats_cl = [f.contiguous().to(dt) for f in feats_cl]
    loc, w = loc.contiguous().to(dt), w.contiguous().to(dt)
    S, N = feats_cl[0].shape[:2]
    C = feats_cl[0].shape[-1]
    _, Q, P, _ = loc.shape
    L = len(feats_cl)
    out = torch.empty(S, Q, C, P, dtype=dt)
    ptrs = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats_cl])
    hw = (ctypes.c_int32 * (2 * L))(*[int(x) for f in feats_cl for x in f.shape[2:4]])
    fn = lib.oracle_msmv_fwd_f64 if dt == torch.float64 else lib.oracle_msmv_fwd
    rc = fn(ptrs, hw, L, ctypes.c_void_p(loc.data_ptr()),
                             ctypes.c_void_p(w.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                             S, N, Q, P, C)
    assert rc == 0
    return out


def msda_torch(value, shapes, starts, loc, attn, f32_coords=False):
    """Pure-torch MSDA with Deformable-DETR kernel semantics (align_corners=False), in the operands' dtype.
    ``f32_coords``: see ``_coord``."""
    bs, keys, heads, dim = value.shape
    _, Q, _, L, P, _ = loc.shape
    out = torch.zeros(bs, Q, heads, dim, dtype=torch.promote_types(value.dtype, loc.dtype))
    for b in range(bs):
        for h in range(heads):
            for l in range(L):
                H, W = int(shapes[l][0]), int(shapes[l][1])
                st = int(starts[l])
                fmap = value[b, st:st + H * W, h].reshape(H, W, dim)
                x = loc[b, :, h, l, :, 0].reshape(-1)
                y = loc[b, :, h, l, :, 1].reshape(-1)
                h_im, w_im = _coord(y, H, 0.5, f32_coords), _coord(x, W, 0.5, f32_coords)
                guard = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
                val = _bilinear_taps(fmap, h_im, w_im) * guard[:, None].float()
                val = val * attn[b, :, h, l].reshape(-1)[:, None]
                out[b, :, h] += val.reshape(Q, P, dim).sum(1)
    return out.reshape(bs, Q, heads * dim)


def msda(value, shapes, starts, loc, attn, force_torch=False):
    """MultiScaleDeformableAttnFunction_fp32.forward contract
    (models/multi_scale_deformable_attn_function.py:93-128)."""
    lib = None if force_torch else _clib()
    if lib is None:
        return msda_torch(value, shapes, starts, loc, attn)
    dt = torch.float64 if value.dtype == torch.float64 else torch.float32
    value, loc, attn = value.contiguous().to(dt), loc.contiguous().to(dt), attn.contiguous().to(dt)
    shapes = torch.as_tensor(shapes, dtype=torch.int64).contiguous()
    starts = torch.as_tensor(starts, dtype=torch.int64).contiguous()
    bs, keys, heads, dim = value.shape
    _, Q, _, L, P, _ = loc.shape
    out = torch.empty(bs, Q, heads * dim, dtype=dt)
    fn = lib.oracle_msda_fwd_f64 if dt == torch.float64 else lib.oracle_msda_fwd
    rc = fn(ctypes.c_void_p(value.data_ptr()), ctypes.c_void_p(shapes.data_ptr()),
                             ctypes.c_void_p(starts.data_ptr()), ctypes.c_void_p(loc.data_ptr()),
                             ctypes.c_void_p(attn.data_ptr()), ctypes.c_void_p(out.data_ptr()),
                             bs, keys, heads, dim, Q, L, P)
    assert rc == 0
    return out


# =============================================================================== sampling_4d
LOC_TAP = None   # set to a list by a test to collect every sampling_4d call's (u, v, view / (N-1)) locations
VIEW_FORCE = None  # a list of u8 [S,Q,P] arrays, consumed one per sampling_4d call: camera index imposed on every point


def views_of(loc, num_cams):
    """camera index per sampling point from the third location coordinate (sparsebev_sampling.py:110)."""
    return torch.round(loc[..., 2] * (num_cams - 1)).to(torch.uint8)


def project_select(points, lidar2img, image_h, image_w, eps=1e-5, force_view=None):
    """models/sparsebev_sampling.py:45-110.  points [B,Q,T,GP,3]; lidar2img [B,T*N,4,4].
    Returns loc [B,T,Q,GP,3] = (u, v, i_view/(N-1)), i_view [B,T,Q,GP], valid-any [B,T,Q,GP].
    ``force_view`` [B,T,Q,GP] (tests): take this camera for every point instead of the first valid one."""
    B, Q, T, GP, _ = points.shape
    N = lidar2img.shape[1] // T
    m = lidar2img.reshape(B, T, N, 1, 1, 4, 4)
    p = points.permute(0, 2, 1, 3, 4)[:, :, None]              # [B,T,1,Q,GP,3]
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    cam = [m[..., i, 0] * x + m[..., i, 1] * y + m[..., i, 2] * z + m[..., i, 3] for i in range(3)]
    homo = cam[2]
    hz = torch.maximum(homo, torch.zeros_like(homo) + eps)
    u = cam[0] / hz / image_w
    v = cam[1] / hz / image_h
    valid = (homo > eps) & (v > 0.0) & (v < 1.0) & (u > 0.0) & (u < 1.0)   # [B,T,N,Q,GP]
    validf = valid.float().permute(0, 1, 3, 4, 2)              # [B,T,Q,GP,N]
    i_view = own_view = torch.argmax(validf, dim=-1)           # first valid, 0 if none
    if force_view is not None:
        i_view = force_view.long()
    idx = i_view[..., None]
    u_sel = torch.gather(u.permute(0, 1, 3, 4, 2), -1, idx)[..., 0]
    v_sel = torch.gather(v.permute(0, 1, 3, 4, 2), -1, idx)[..., 0]
    loc = torch.stack([u_sel, v_sel, i_view.float() / (N - 1)], dim=-1)
    if LOC_TAP is not None:   # tests: (u, v) as sampled + this implementation's OWN camera choice, slot-major [S,Q,P,3]
        LOC_TAP.append(torch.stack([u_sel, v_sel, own_view.float() / (N - 1)], dim=-1))
    return loc, i_view, valid.any(dim=2)


def sampling_4d(sample_points, feats_cl, scale_weights, lidar2img, image_h, image_w, eps=1e-5):
    """models/sparsebev_sampling.py:28-134 with the msmv op in kernel semantics.
    sample_points [B,Q,T,G,P,3]; feats_cl[l] [B*T*G,N,H,W,C]; scale_weights [B,Q,G,T,P,L].
    Slot order of points/features/outputs is (b,t,g); the weights are flattened (b,g,t)
    (:118-120) and consumed slot-by-slot as they lie -- reproduced as written (quirk Q1)."""
    B, Q, T, G, P, _ = sample_points.shape
    force = None
    if VIEW_FORCE:
        force = torch.as_tensor(np.asarray(VIEW_FORCE.pop(0))).view(B, T, G, Q, P).permute(0, 1, 3, 2, 4).reshape(B, T, Q, G * P)
    loc, _, _ = project_select(sample_points.reshape(B, Q, T, G * P, 3), lidar2img, image_h,
                               image_w, eps, force)
    loc = loc.reshape(B, T, Q, G, P, 3).permute(0, 1, 3, 2, 4, 5).reshape(B * T * G, Q, P, 3)
    if LOC_TAP is not None:           # (project_select appended [B,T,Q,GP,3]: bring it to the op's slot order [S,Q,P,3])
        LOC_TAP[-1] = LOC_TAP[-1].reshape(B, T, Q, G, P, 3).permute(0, 1, 3, 2, 4, 5).reshape(B * T * G, Q, P, 3)
    L = scale_weights.shape[-1]
    w = scale_weights.reshape(B, Q, G, T, P, L).permute(0, 2, 3, 1, 4, 5).reshape(B * G * T, Q, P, L)
    out = msmv_gather(feats_cl, loc.contiguous(), w.contiguous())      # [S,Q,C,P]
    C = out.shape[2]
    out = out.reshape(B, T, G, Q, C, P).permute(0, 3, 2, 1, 5, 4)       # [B,Q,G,T,P,C]
    return out.flatten(3, 4)


# =============================================================================== layers
def _lin(sd, name, x):
    return F.linear(x, sd[name + ".weight"], sd.get(name + ".bias"))


def _ln(sd, name, x):
    return F.layer_norm(x, (x.shape[-1],), sd[name + ".weight"], sd[name + ".bias"])


def _sub(sd, prefix):
    n = len(prefix)
    return {k[n:]: v for k, v in sd.items() if k.startswith(prefix)}


def time_diff_from_metas(img_metas, B, num_cams):
    """models/racformer_transformer.py:99-103 (float64 numpy, mean over cams, cast f32)."""
    ts = np.array([m["img_timestamp"] for m in img_metas], dtype=np.float64)
    ts = np.reshape(ts, [B, -1, num_cams])
    td = np.mean(ts[:, :1, :] - ts, axis=-1).astype(np.float32)
    return torch.from_numpy(td)


def regroup_pyramid(mlvl_feats, num_cams, groups=4):
    """models/racformer_transformer.py:112-124, channel-last branch:
    [B,T*N,G*C,H,W] -> [B*T*G, N, H, W, C]."""
    out = []
    for f in mlvl_feats:
        B, TN, GC, H, W = f.shape
        N, T, C = num_cams, TN // num_cams, GC // groups
        f = f.reshape(B, T, N, groups, C, H, W).permute(0, 1, 3, 2, 5, 6, 4)
        out.append(f.reshape(B * T * groups, N, H, W, C).contiguous())
    return out


def position_encoder(sd, x):
    """models/racformer_transformer.py:170-177"""
    x = F.relu(_ln(sd, "position_encoder.1", _lin(sd, "position_encoder.0", x)))
    return F.relu(_ln(sd, "position_encoder.4", _lin(sd, "position_encoder.3", x)))


def sasa(sd, query_bbox, query_feat, pc_range, num_heads=8):
    """ScaleAdaptiveSelfAttention.inner_forward + calc_bbox_dists
    (models/racformer_transformer.py:296-335) over mmcv MultiheadAttention(batch_first) =
    identity + nn.MultiheadAttention(q,q,q, float attn_mask)[0] (need_weights path: q is
    pre-scaled by 1/sqrt(d), mask added to the logits, softmax, AV, out_proj)."""
    B, Q, E = query_feat.shape
    centers = decode_bbox(theta_d2xy(query_bbox), pc_range)[..., :2]
    dist = -torch.norm(centers[:, :, None, :] - centers[:, None, :, :], dim=-1)     # [B,Q,Q]
    tau = _lin(sd, "self_attn.gen_tau", query_feat).permute(0, 2, 1)               # [B,8,Q]
    mask = dist[:, None] * tau[..., None]                                          # [B,8,Q,Q]
    d = E // num_heads
    qkv = F.linear(query_feat, sd["self_attn.attention.attn.in_proj_weight"],
                   sd["self_attn.attention.attn.in_proj_bias"])
    q, k, v = qkv.split(E, dim=-1)

    def heads(t):
        return t.reshape(B, Q, num_heads, d).permute(0, 2, 1, 3)

    q, k, v = heads(q) * math.sqrt(1.0 / d), heads(k), heads(v)
    logits = mask + q @ k.transpose(-1, -2)
    p = torch.softmax(logits, dim=-1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(B, Q, E)
    o = _lin(sd, "self_attn.attention.attn.out_proj", o)
    return query_feat + o


def _ray_depth_offsets(sd, prefix, query_feat, d_region, depth_num):
    """racformer_transformer.py:395-396 / :515-516"""
    base = torch.linspace(-d_region, d_region, depth_num).view(1, 1, depth_num)
    jit = (torch.sigmoid(_lin(sd, prefix + ".ray_points_offset", query_feat)) * 2 - 1)
    return base + jit * d_region / depth_num / 2


def image_keypoints(sd, query_ray, query_feat, time_diff, d_region, cfg):
    """RaCFormerSampling.inner_forward up to the sampling call
    (models/racformer_transformer.py:361-408).  Returns points [B,Q,T,G,P,3] (metric xyz) and
    scale weights [B,Q,G,T,P,L]."""
    B, Q, _ = query_ray.shape
    T, G, NP, D, L = cfg.num_frames, cfg.num_groups, cfg.num_points, cfg.img_depth_num, cfg.num_levels
    pc = cfg.pc_range
    qb = theta_d2xy(query_ray)
    off = _lin(sd, "sampling.sampling_offset", query_feat).view(B, Q, G * NP * D, 3)
    pts = make_sample_points(qb, off, pc).reshape(B, Q, 1, G, NP * D, 3)
    pts = pts.expand(B, Q, T, G, NP * D, 3)
    shift = (query_ray[..., 8:][:, :, None, :] * time_diff[:, None, :, None])[:, :, :, None, None, :]
    xy = pts[..., 0:2] - shift
    x = (xy[..., 0:1] - pc[0]) / (pc[3] - pc[0])
    y = (xy[..., 1:2] - pc[1]) / (pc[4] - pc[1])
    polar = xy2theta_d(torch.cat([x, y, pts[..., 2:3]], dim=-1))
    polar = polar.reshape(B, Q, T, G, NP, D, 3)
    d_off = _ray_depth_offsets(sd, "sampling", query_feat, d_region, D).view(B, Q, 1, 1, 1, D, 1)
    polar = torch.cat([polar[..., 0:1], polar[..., 1:2] + d_off, polar[..., 2:]], dim=-1)
    polar = polar.reshape(B, Q, T, G, NP * D, 3)
    out = theta_d2xy(polar)
    px = out[..., 0:1] * (pc[3] - pc[0]) + pc[0]
    py = out[..., 1:2] * (pc[4] - pc[1]) + pc[1]
    points = torch.cat([px, py, out[..., 2:]], dim=-1)
    sw = _lin(sd, "sampling.scale_weights", query_feat).view(B, Q, G, T, D * NP, L)
    return points, torch.softmax(sw, dim=-1)


def bev_keypoints(sd, prefix, query_ray, query_feat, time_diff, d_region, cfg, heads=4):
    """BEVSampling.inner_forward up to the attention call
    (models/racformer_transformer.py:490-529).  Returns loc [B,Q,heads,T,P,2] in [0,1] and
    weights [B,Q,heads,T,1,P]."""
    B, Q, _ = query_ray.shape
    T, NP, D = cfg.num_frames, cfg.num_points_bev, cfg.bev_depth_num
    pc = cfg.pc_range
    qb = theta_d2xy(query_ray)
    off = _lin(sd, prefix + ".sampling_offset", query_feat).view(B, Q, heads * NP * D, 2)
    off = torch.cat([off, torch.zeros_like(off[..., 0:1])], dim=-1)
    pts = make_sample_points(qb, off, pc).reshape(B, Q, 1, heads, NP * D, 3)
    pts = pts.expand(B, Q, T, heads, NP * D, 3)
    shift = (query_ray[..., 8:][:, :, None, :] * time_diff[:, None, :, None])[:, :, :, None, None, :]
    xy = pts[..., 0:2] - shift
    x = (xy[..., 0:1] - pc[0]) / (pc[3] - pc[0])
    y = (xy[..., 1:2] - pc[1]) / (pc[4] - pc[1])
    polar = xy2theta_d(torch.cat([x, y], dim=-1)).reshape(B, Q, T, heads, NP, D, 2)
    d_off = _ray_depth_offsets(sd, prefix, query_feat, d_region, D).view(B, Q, 1, 1, 1, D, 1)
    polar = torch.cat([polar[..., 0:1], polar[..., 1:2] + d_off], dim=-1)
    loc = theta_d2xy(polar.reshape(B, Q, T, heads, NP * D, 2))
    loc = loc.permute(0, 1, 3, 2, 4, 5).contiguous()                     # [B,Q,heads,T,P,2]
    sw = _lin(sd, prefix + ".scale_weights", query_feat).view(B, Q, heads, 1, 1, D * NP)
    sw = torch.softmax(sw, dim=-1).expand(B, Q, heads, T, 1, D * NP).contiguous()
    return loc, sw


def learned_pos_encoding(sd, prefix, h, w):
    """mmdet LearnedPositionalEncoding.forward (2.28.2) -> [2*num_feats, h, w]."""
    col = sd[prefix + ".col_embed.weight"][:w]
    row = sd[prefix + ".row_embed.weight"][:h]
    pos = torch.cat([col[None].expand(h, w, -1), row[:, None].expand(h, w, -1)], dim=-1)
    return pos.permute(2, 0, 1)


def conv_gru(sd, prefix, x):
    """ConvGRU / ConvGRUCell (models/racformer_transformer.py:665-720): only the first
    min(4,T) frames are updated; later frames get the zero initial state."""
    B, T, C, H, W = x.shape
    hid = sd[prefix + ".convGRUCell.matching_layer.weight"].shape[1]
    h = torch.zeros(B, hid, H, W)
    outs = []
    for t in range(T):
        if t >= (4 if T > 4 else T):
            outs.append(torch.zeros(B, hid, H, W))
            continue
        hm = F.conv2d(h, sd[prefix + ".convGRUCell.matching_layer.weight"],
                      sd[prefix + ".convGRUCell.matching_layer.bias"])
        gates = F.conv2d(torch.cat([x[:, t], hm], dim=1), sd[prefix + ".convGRUCell.gates_conv.weight"],
                         sd[prefix + ".convGRUCell.gates_conv.bias"], padding=1)
        zg, rg, cand = torch.split(gates, hid, dim=1)
        z, r = torch.sigmoid(zg), torch.sigmoid(rg)
        cand = torch.tanh(cand + r * h)
        h = (1 - z) * h + z * cand
        outs.append(h)
    return torch.stack(outs, dim=1)


def temporal_encoder(sd, prefix, bev):
    """RadarBEVTemporalEncoder.inner_forward (models/racformer_transformer.py:645-656)"""
    B, T, C, H, W = bev.shape
    down = F.conv2d(bev.flatten(0, 1), sd[prefix + ".downsample.weight"], sd[prefix + ".downsample.bias"],
                    stride=2, padding=1)
    hid = down.shape[1]
    down = down.reshape(B, T, hid, H // 2, W // 2)
    hfeat = conv_gru(sd, prefix + ".convGRU", down).flatten(0, 1)
    up = F.interpolate(hfeat, scale_factor=2, mode="bilinear", align_corners=True)
    up = F.conv2d(up, sd[prefix + ".upsample.1.weight"], sd[prefix + ".upsample.1.bias"], padding=1)
    up = up.reshape(B, T, hid, H, W)
    cat = torch.cat([bev, up], dim=2).flatten(0, 1)
    out = F.conv2d(cat, sd[prefix + ".temporal_fusion.weight"], sd[prefix + ".temporal_fusion.bias"],
                   padding=1)
    return out.reshape(B, T, C, H, W)


def bev_self_attention(sd, prefix, query, value_maps, loc, attn_w, heads=4):
    """BEVSelfAttention.forward (models/bev_self_attention.py:115-225).  value_maps [B,T,C,H,W]
    (already bev+pos); loc [B,Q,heads,T,P,2]; attn_w [B,Q,heads,T,1,P].  Quirk Q2: loc/attn are
    flattened frame-major (t*B+b), values batch-major (b*T+t) -- as written."""
    B, Q, C = query.shape
    T, H, W = value_maps.shape[1], value_maps.shape[3], value_maps.shape[4]
    P = loc.shape[-2]
    value = value_maps.reshape(B * T, C, H * W).permute(0, 2, 1)
    value = _lin(sd, prefix + ".value_proj", value).reshape(B * T, H * W, heads, C // heads)
    loc7 = loc.view(B, Q, heads, T, 1, P, 2).permute(3, 0, 1, 2, 4, 5, 6).reshape(B * T, Q, heads, 1, P, 2)
    aw = attn_w.view(B, Q, heads, T, 1, P).permute(3, 0, 1, 2, 4, 5).reshape(B * T, Q, heads, 1, P)
    out = msda(value.contiguous(), [[H, W]], [0], loc7.contiguous(), aw.contiguous())   # [B*T,Q,C]
    out = out.permute(1, 2, 0).reshape(Q, C, B, T)
    qw = _lin(sd, prefix + ".bev_queue_weight", query).permute(1, 0, 2).reshape(Q, 1, B, T)
    out = torch.sum(out * torch.softmax(qw, dim=-1), dim=-1).permute(2, 0, 1)
    return _lin(sd, prefix + ".output_proj", out) + query


def bev_sampling(sd, prefix, query_ray, query_feat, bev, time_diff, d_region, cfg, temp_radar):
    """BEVSampling.inner_forward (models/racformer_transformer.py:479-539)"""
    if temp_radar:
        bev = temporal_encoder(sd, prefix + ".temporal_encoder", bev)
    H, W = bev.shape[-2:]
    loc, sw = bev_keypoints(sd, prefix, query_ray, query_feat, time_diff, d_region, cfg)
    pos = learned_pos_encoding(sd, prefix + ".positional_encoding", H, W)
    return bev_self_attention(sd, prefix + ".attention", query_feat, bev + pos[None, None], loc, sw)


def adaptive_mixing(sd, x, query, n_groups=4, out_points=128):
    """AdaptiveMixing.inner_forward (models/racformer_transformer.py:580-610)"""
    B, Q, G, P, C = x.shape
    params = _lin(sd, "mixing.parameter_generator", query).reshape(B * Q, G, -1)
    M, S = params.split([C * C, P * out_points], 2)
    M = M.reshape(B * Q, G, C, C)
    S = S.reshape(B * Q, G, out_points, P)
    out = torch.matmul(x.reshape(B * Q, G, P, C), M)
    out = F.relu(F.layer_norm(out, [P, C]))
    out = torch.matmul(S, out)
    out = F.relu(F.layer_norm(out, [out_points, C]))
    out = _lin(sd, "mixing.out_proj", out.reshape(B, Q, -1))
    return query + out


def ffn(sd, x):
    """mmcv FFN(256, 512) with identity (racformer_transformer.py:187,258)"""
    return x + _lin(sd, "ffn.layers.1", F.relu(_lin(sd, "ffn.layers.0.0", x)))


def cls_branch(sd, x):
    x = F.relu(_ln(sd, "cls_branch.1", _lin(sd, "cls_branch.0", x)))
    x = F.relu(_ln(sd, "cls_branch.4", _lin(sd, "cls_branch.3", x)))
    return _lin(sd, "cls_branch.6", x)


def reg_branch(sd, x):
    x = F.relu(_lin(sd, "reg_branch.0", x))
    x = F.relu(_lin(sd, "reg_branch.2", x))
    return _lin(sd, "reg_branch.4", x)


def refine_bbox(proposal, delta, num_ray):
    """models/racformer_transformer.py:230-236"""
    dz = torch.sigmoid(delta[..., 1:3] + inverse_sigmoid(proposal[..., 1:3]))
    theta = proposal[..., 0:1] + (torch.sigmoid(delta[..., 0:1]) * 2 - 1) / num_ray
    return torch.cat([theta, dz, delta[..., 3:]], dim=-1)


def decoder_layer(sd, query_bbox, query_feat, feats_cl, lss_bev, radar_bev, time_diff, lidar2img,
                  cfg, layer, stages=None):
    """RaCFormerTransformerDecoderLayer.forward (models/racformer_transformer.py:239-279).
    ``sd`` holds keys relative to ``...decoder.decoder_layer.``."""
    d_region = cfg.d_region_list[layer]
    pos = position_encoder(sd, query_bbox[..., :3])
    q = query_feat + pos
    sa = sasa(sd, query_bbox, q, cfg.pc_range)
    q = _ln(sd, "norm1", sa)
    radar_raw = bev_sampling(sd, "sampling_radar_bev", query_bbox, q, radar_bev, time_diff, d_region,
                             cfg, True)
    radar = _ln(sd, "norm_radar_bev", radar_raw)
    lss_raw = bev_sampling(sd, "sampling_lss_bev", query_bbox, q, lss_bev, time_diff, d_region, cfg,
                           False)
    lss = _ln(sd, "norm_lss_bev", lss_raw)
    pts, sw = image_keypoints(sd, query_bbox, q, time_diff, d_region, cfg)
    sampled = sampling_4d(pts, feats_cl, sw, lidar2img, cfg.image_hw[0], cfg.image_hw[1])
    mixed = adaptive_mixing(sd, sampled, q)
    q = _ln(sd, "norm2", mixed)
    q = _ln(sd, "norm_fusion", _lin(sd, "fusion", torch.cat([q, radar, lss], dim=-1)))
    ffn_out = ffn(sd, q)
    q = _ln(sd, "norm3", ffn_out)
    cls = cls_branch(sd, q)
    box = refine_bbox(query_bbox, reg_branch(sd, q), cfg.num_ray)
    if time_diff.shape[1] > 1:
        td = time_diff.clone()
        td[td < 1e-5] = 1.0
        box = torch.cat([box[..., :8], box[..., 8:] / td[:, 1:2, None]], dim=-1)
    if stages is not None:
        stages.update(position_encoder=pos, self_attn=sa, sampling_radar_bev=radar_raw,
                      sampling_lss_bev=lss_raw, sampling=sampled, mixing=mixed, ffn=ffn_out)
    return q, cls, box


def transformer_forward(sd, query_bbox, query_feat, mlvl_feats, lss_bev, radar_bev, img_metas, cfg,
                        stages_per_layer=None):
    """RaCFormerTransformer.forward + RaCFormerTransformerDecoder.forward
    (models/racformer_transformer.py:52-58, 95-142).  ``sd``: keys with the
    ``decoder.decoder_layer.`` prefix (a RaCFormerTransformer state_dict)."""
    lsd = _sub(sd, "decoder.decoder_layer.")
    B = query_bbox.shape[0]
    time_diff = time_diff_from_metas(img_metas, B, cfg.num_cams)
    lidar2img = torch.from_numpy(np.asarray([m["lidar2img"] for m in img_metas]).astype(np.float32))
    feats_cl = regroup_pyramid(mlvl_feats, cfg.num_cams, cfg.num_groups)
    cls_all, box_all = [], []
    for i in range(cfg.num_layers):
        st = {} if stages_per_layer is not None else None
        query_feat, cls, box = decoder_layer(lsd, query_bbox, query_feat, feats_cl, lss_bev, radar_bev,
                                             time_diff, lidar2img, cfg, i, st)
        if stages_per_layer is not None:
            stages_per_layer.append(st)
        query_bbox = box.clone()
        cls_all.append(cls)
        box_all.append(theta_d2xy(box))
    return torch.nan_to_num(torch.stack(cls_all)), torch.nan_to_num(torch.stack(box_all))


# =============================================================================== head / decode
def head_forward(head_sd, tr_sd, mlvl_feats, lss_bev, radar_bev, img_metas, cfg):
    """RaCFormer_head.forward, inference branch (models/racformer_head.py:82-134, 136-145).
    Pinned by tests/golden/head_small6.npz / head_f8.npz."""
    B = lss_bev.shape[0]
    Q = cfg.num_query
    qb = head_sd["init_query_bbox.weight"].clone().view(1, Q, 10).repeat(B, 1, 1)
    feat = head_sd["label_enc.weight"][cfg.num_classes].repeat(Q, 1)
    qf = torch.cat([feat, torch.zeros(Q, 1)], dim=1).repeat(B, 1, 1)
    cls, box = transformer_forward(tr_sd, qb, qf, mlvl_feats, lss_bev, radar_bev, img_metas, cfg)
    pc = cfg.pc_range
    box = box.clone()
    box[..., 0] = box[..., 0] * (pc[3] - pc[0]) + pc[0]
    box[..., 1] = box[..., 1] * (pc[4] - pc[1]) + pc[1]
    box[..., 2] = box[..., 2] * (pc[5] - pc[2]) + pc[2]
    box = torch.cat([box[..., 0:2], box[..., 3:5], box[..., 2:3], box[..., 5:10]], dim=-1)
    return dict(all_cls_scores=cls, all_bbox_preds=box)


def head_init_query(num_query, num_clusters):
    """RaCFormer_head._init_layers + generate_points (models/racformer_head.py:51-79): the deterministic columns of
    ``init_query_bbox.weight`` -- (theta, d) on a polar grid of num_query // num_clusters rays x num_clusters ranges
    (row-major ray, range), z = 0.5, log h = 0.2, velocity 0.  Columns 3, 4, 6, 7 keep nn.Embedding's N(0,1) draw and are
    returned as NaN.  -> [num_query, 10]."""
    rays = num_query // num_clusters
    ang = torch.linspace(0, 1, rays + 1)[:-1]
    dist = torch.linspace(0, 1, num_clusters + 2, dtype=torch.float)[1:-1]
    w = torch.full((num_query, 10), float("nan"))
    w[:, 0] = ang.view(rays, 1).expand(rays, num_clusters).reshape(-1)
    w[:, 1] = dist.view(1, num_clusters).expand(rays, num_clusters).reshape(-1)
    w[:, 2], w[:, 5], w[:, 8:10] = 0.5, 0.2, 0.0
    return w


def nms_free_decode(cls_scores, bbox_preds, max_num=300, num_classes=10, score_threshold=0.05,
                    post_center_range=(-61.2, -61.2, -10.0, 61.2, 61.2, 10.0), z_bottom=True):
    """NMSFreeCoder.decode_single (models/bbox/coders/nms_free_coder.py:37-88) and, with ``z_bottom``, the shift of z to
    the box bottom that RaCFormer_head.get_bboxes applies (models/racformer_head.py:488-496).
    cls_scores [Q,C] logits, bbox_preds [Q,10] of the LAST layer.  ``score_threshold`` follows the reference's two
    tests: the mask is computed when it ``is not None`` (:61) but only applied when it is truthy (:69), so 0.0 filters
    nothing.  Pinned by tests/golden/decode_cases.npz."""
    scores, idx = cls_scores.sigmoid().view(-1).topk(max_num)
    labels = idx % num_classes
    bidx = torch.div(idx, num_classes, rounding_mode="trunc")
    boxes = denormalize_bbox(bbox_preds[bidx])
    lim = torch.tensor(post_center_range)
    mask = (boxes[..., :3] >= lim[:3]).all(1) & (boxes[..., :3] <= lim[3:]).all(1)
    if score_threshold:
        mask &= scores > score_threshold
    boxes, scores, labels = boxes[mask], scores[mask], labels[mask]
    boxes = boxes.clone()
    if z_bottom:
        boxes[:, 2] = boxes[:, 2] - boxes[:, 5] * 0.5
    return dict(bboxes=boxes, scores=scores, labels=labels, query_index=bidx[mask])


# =============================================================================== bev_pool_v2 (row f2)
def bev_pool_v2(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape, interval_starts, interval_lengths):
    """BEVPoolv2 forward restated from models/csrc/bev_pool_v2/src/bev_pool_cuda.cu:21-48 with plain torch
    indexing (differentiable, so autograd of this function is the oracle for the backward kernel too):
    out[ranks_bev[start_s]] = sum_{i in interval s} depth[ranks_depth[i]] * feat[ranks_feat[i]].
    Returns [B, C, Z, Y, X] like bev_pool.py:87-92.  PINNED by the reference's inline known-answer vectors
    (tests/golden/bev_pool_known_answer.json)."""
    c = feat.shape[-1]
    contrib = feat.reshape(-1, c)[ranks_feat.long()] * depth.reshape(-1)[ranks_depth.long()][:, None]
    seg = torch.repeat_interleave(torch.arange(interval_starts.shape[0]), interval_lengths.long())
    sums = torch.zeros(interval_starts.shape[0], c, dtype=contrib.dtype).index_add(0, seg, contrib)
    out = torch.zeros(int(np.prod(bev_feat_shape[:-1])), c, dtype=contrib.dtype)
    out = out.index_copy(0, ranks_bev.long()[interval_starts.long()], sums)
    return out.reshape(*bev_feat_shape).permute(0, 4, 1, 2, 3).contiguous()
