"""float64 torch restatements around rac_bev_sampling_fwd / rac_bev_sampling_bwd (test helper, no GPU):

  chain64          the kernel's keypoint chain from the box table on (B == 1), differentiable: loc [Q,heads,T,P,2], aw, qw
  core64           the whole forward (chain + bilinear gather + both softmaxes) -> out [1,Q,heads*64] (and loc)
  gather_grads     the gather half of the backward in closed form at given locations (what rac_msda_bwd computes per keypoint)
  closed_form_bwd  the backward the kernel implements, formula by formula (no autograd): every output of its table
  fake_fused / fake_backward   drop-in fakes of the two launchers of racformer_amd.fused for CPU plumbing tests
"""
import math

import torch

from racformer_amd.transformer import box_table_torch

TWO_PI = 2 * math.pi


def _f64(x):
    return x.detach().double()


def depth_base(d_region, D):
    return torch.linspace(-d_region, d_region, D).double()     # (formed in float32 as the launcher forms it)


def chain64(box, vel, off, ray, time_diff, heads, NP, D, pc, d_region, clamp=True, dtype=torch.float64):
    """box [Q,8], vel [Q,2], off [Q,heads*P*2], ray [Q,D], time_diff [T] -> loc [Q,heads,T,P,2] (in ``dtype``, on ray's device)."""
    Q, P, T = box.shape[0], NP * D, time_diff.shape[0]
    o = off.reshape(Q, heads, P, 2)
    dx, dy = box[:, 3, None, None] * o[..., 0], box[:, 4, None, None] * o[..., 1]
    cs, sn = box[:, 6, None, None], box[:, 7, None, None]
    bx = box[:, 0, None, None] + (dx * cs - dy * sn)
    by = box[:, 1, None, None] + (dx * sn + dy * cs)                       # [Q,heads,P]
    px = bx[:, :, None, :] - (vel[:, 0, None] * time_diff[None, :])[:, None, :, None]
    py = by[:, :, None, :] - (vel[:, 1, None] * time_diff[None, :])[:, None, :, None]   # [Q,heads,T,P]
    ex = (px - pc[0]) / (pc[3] - pc[0]) * 102.4 - 51.2
    ey = (py - pc[1]) / (pc[4] - pc[1]) * 102.4 - 51.2
    doff = depth_base(d_region, D).to(device=ray.device, dtype=dtype) + (torch.sigmoid(ray) * 2 - 1) * d_region / D / 2     # [Q,D]
    doff = doff.repeat(1, NP)[:, None, None, :]                                          # p % D
    dist = torch.sqrt(ex * ex + ey * ey) / 65.0 + doff
    ang = torch.remainder(torch.atan2(ey, ex) + TWO_PI, TWO_PI)
    rad = dist * 65.0
    loc = torch.stack([(51.2 + rad * torch.cos(ang)) / 102.4, (51.2 + rad * torch.sin(ang)) / 102.4], dim=-1)
    return loc.clamp(0, 1) if clamp else loc


def _taps(loc, H, W, f32_coords):
    """loc [...,2] -> list of (pixel index, weight, d weight / d h_im, d weight / d w_im, ok) with MSDA semantics"""
    x, y = loc[..., 0], loc[..., 1]
    if f32_coords:     # the pixel coordinate rounded operation by operation in float32, as the kernels form it
        h_im = ((y.float() * H) - 0.5).double() + (y - y.detach()) * H
        w_im = ((x.float() * W) - 0.5).double() + (x - x.detach()) * W
    else:
        h_im, w_im = y * H - 0.5, x * W - 0.5
    guard = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
    hs, ws = torch.where(guard, h_im, torch.zeros_like(h_im)), torch.where(guard, w_im, torch.zeros_like(w_im))
    hl, wl = torch.floor(hs.detach()), torch.floor(ws.detach())
    lh, lw = hs - hl, ws - wl
    hh, hw = 1 - lh, 1 - lw
    out = []
    for a, b, tw, dh, dw in ((0, 0, hh * hw, -hw, -hh), (0, 1, hh * lw, -lw, hh), (1, 0, lh * hw, hw, -lh), (1, 1, lh * lw, lw, lh)):
        hi, wi = hl.long() + a, wl.long() + b
        ok = guard & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
        out.append((hi.clamp(0, H - 1) * W + wi.clamp(0, W - 1), tw, dh, dw, ok))
    return out


def _tap_values(value, idx, heads):
    """value [T,HW,heads,64], idx [Q,heads,T,P] -> [Q,heads,T,P,64]"""
    Q, Hn, T, P = idx.shape
    t_i = torch.arange(T)[None, None, :, None].expand_as(idx)
    h_i = torch.arange(Hn)[None, :, None, None].expand_as(idx)
    return value[t_i, idx, h_i]


def sampled64(value, loc, hw, f32_coords=False, magnitude=False):
    """bilinear(V[t], loc[q,h,t,p])[h] -> [Q,heads,T,P,64], differentiable in value and loc.  magnitude: |value| under |tap weight|,
    the scale A of a forward's error bound"""
    H, W = hw
    s = 0
    if magnitude:
        value = value.abs()
    for idx, tw, _, _, ok in _taps(loc, H, W, f32_coords):
        s = s + _tap_values(value, idx, loc.shape[1]) * ((tw.abs() if magnitude else tw) * ok)[..., None]
    return s


def core64(value, hw, query_bbox, off, ray, sc, qu, time_diff, T, heads, NP, D, pc, d_region, box_table=None, f32_coords=False):
    """float64 forward of rac_bev_sampling_fwd for B == 1 -> (out [1,Q,heads*64], loc [1,Q,heads,T,P,2])"""
    assert query_bbox.shape[0] == 1
    Q, P = query_bbox.shape[1], NP * D
    qb = query_bbox.double()
    box = (box_table_torch(qb, pc) if box_table is None else box_table.double())[0]
    loc = chain64(box, qb[0, :, 8:10].detach(), off.double()[0], ray.double()[0], time_diff.double()[0], heads, NP, D, pc, d_region)
    aw = torch.softmax(sc.double()[0].reshape(Q, heads, P), dim=-1)
    qw = torch.softmax(qu.double()[0], dim=-1)
    locb = loc[None]            # (returned; a caller may retain its gradient: the sampling goes through it)
    smp = sampled64(value.double(), locb[0], hw, f32_coords)
    out = (smp * (aw[:, :, None, :] * qw[:, None, :, None])[..., None]).sum((2, 3))
    return out.reshape(1, Q, heads * 64), locb


def gather_grads(value, loc, wgt, gout, hw, f32_coords=False):
    """value [T,HW,heads,64], loc [Q,heads,T,P,2], wgt [Q,heads,T,P], gout [Q,heads,64] (all float64) ->
    grad_value, grad_loc (weight included), grad_attn (per unit weight): the closed form of rac_msda_bwd"""
    H, W = hw
    Q, Hn, T, P, _ = loc.shape
    gv = torch.zeros_like(value)
    g = gout[:, :, None, None, :]
    sv, sh, sw = 0, 0, 0
    t_i = torch.arange(T)[None, None, :, None].expand(Q, Hn, T, P)
    h_i = torch.arange(Hn)[None, :, None, None].expand(Q, Hn, T, P)
    for idx, tw, dh, dw, ok in _taps(loc, H, W, f32_coords):
        v = _tap_values(value, idx, Hn) * ok[..., None]
        dot = (v * g).sum(-1)
        sv, sh, sw = sv + tw * dot, sh + dh * dot, sw + dw * dot
        gv.index_put_((t_i, idx, h_i), ((tw * wgt * ok)[..., None] * g).expand(Q, Hn, T, P, 64), accumulate=True)
    return gv, torch.stack([W * sw * wgt, H * sh * wgt], dim=-1), sv


def closed_form_bwd(value, hw, query_bbox, off, ray, sc, qu, time_diff, gout, T, heads, NP, D, pc, d_region, box_table=None,
                    f32_coords=False, loc_at=None, magnitude=False):
    """The backward rac_bev_sampling_bwd implements, in float64 without autograd -> dict of every output of its table
    (grad_value [T,HW,heads,64], grad_offsets [1,Q,heads*P*2], grad_ray [1,Q,D], grad_scale [1,Q,heads*P], grad_queue [1,Q,T],
    grad_box [1,Q,8], grad_loc [1,Q,heads,T,P,2], grad_attn [1,Q,heads,T,P]).
    ``loc_at`` [1,Q,heads,T,P,2]: gather at these locations (a forward's own loc_out) instead of the float64 chain's, so that the
    taps are that forward's; the chain tail stays the float64 Jacobian.  ``magnitude``: the same sums with every term made
    non-negative (|value|, |grad_out|, |coefficients|): the scale A of an error bound for each output."""
    ab = (lambda x: x.abs()) if magnitude else (lambda x: x)
    sub = (lambda x, y: x + y) if magnitude else (lambda x, y: x - y)
    with torch.no_grad():
        Q, P = query_bbox.shape[1], NP * D
        qb = _f64(query_bbox)
        box = (box_table_torch(qb, pc) if box_table is None else _f64(box_table))[0]
        vel, o, td = qb[0, :, 8:10], _f64(off)[0].reshape(Q, heads, P, 2), _f64(time_diff)[0]
        sg = torch.sigmoid(_f64(ray)[0])
        aw = torch.softmax(_f64(sc)[0].reshape(Q, heads, P), dim=-1)
        qw = torch.softmax(_f64(qu)[0], dim=-1)
        loc = chain64(box, vel, _f64(off)[0], _f64(ray)[0], td, heads, NP, D, pc, d_region) if loc_at is None else _f64(loc_at)[0]
        wgt = aw[:, :, None, :] * qw[:, None, :, None]
        if magnitude:
            gv, gloc, gattn = gather_magnitudes(_f64(value), loc, wgt, _f64(gout)[0].reshape(Q, heads, 64), hw, f32_coords)
        else:
            gv, gloc, gattn = gather_grads(_f64(value), loc, wgt, _f64(gout)[0].reshape(Q, heads, 64), hw, f32_coords)
        # chain tail per keypoint (bev_warp_bwd)
        bw, bl, cs, sn = (box[:, i, None, None] for i in (3, 4, 6, 7))
        dx, dy = bw * o[..., 0], bl * o[..., 1]
        bx = box[:, 0, None, None] + (dx * cs - dy * sn)
        by = box[:, 1, None, None] + (dx * sn + dy * cs)
        sx, sy = pc[3] - pc[0], pc[4] - pc[1]
        px = bx[:, :, None, :] - (vel[:, 0, None] * td[None, :])[:, None, :, None]
        py = by[:, :, None, :] - (vel[:, 1, None] * td[None, :])[:, None, :, None]
        ex, ey = (px - pc[0]) / sx * 102.4 - 51.2, (py - pc[1]) / sy * 102.4 - 51.2
        doff = (depth_base(d_region, D) + (sg * 2 - 1) * d_region / D / 2).repeat(1, NP)[:, None, None, :]
        r2 = ex * ex + ey * ey
        r = torch.sqrt(r2)
        ang = torch.remainder(torch.atan2(ey, ex) + TWO_PI, TWO_PI)
        rad = (r / 65.0 + doff) * 65.0
        c, s = torch.cos(ang), torch.sin(ang)
        ux, uy = (51.2 + rad * c) / 102.4, (51.2 + rad * s) / 102.4
        gux = torch.where((ux >= 0) & (ux <= 1), gloc[..., 0] / 102.4, torch.zeros_like(ux))
        guy = torch.where((uy >= 0) & (uy <= 1), gloc[..., 1] / 102.4, torch.zeros_like(uy))
        g_rad = ab(gux * c) + ab(guy * s)
        g_ang = ab(rad) * sub(ab(guy * c), ab(gux * s))
        pos = r2 > 0
        ir, ir2 = torch.where(pos, 1 / r, torch.zeros_like(r)), torch.where(pos, 1 / r2, torch.zeros_like(r))
        gbx = (sub(ab(g_rad * ex * ir), ab(g_ang * ey * ir2)) * 102.4 / sx).sum(2)          # sums over frames: [Q,heads,P]
        gby = ((ab(g_rad * ey * ir) + ab(g_ang * ex * ir2)) * 102.4 / sy).sum(2)
        gdoff = (g_rad * 65.0).sum((1, 2)).reshape(Q, NP, D).sum(1)               # [Q,D]
        g_dx, g_dy = ab(gbx * cs) + ab(gby * sn), sub(ab(gby * cs), ab(gbx * sn))
        goff = torch.stack([ab(bw * g_dx), ab(bl * g_dy)], dim=-1).reshape(1, Q, heads * P * 2)
        gbox = torch.zeros(Q, 8, dtype=torch.float64)
        gbox[:, 0], gbox[:, 1] = gbx.sum((1, 2)), gby.sum((1, 2))
        gbox[:, 3], gbox[:, 4] = ab(o[..., 0] * g_dx).sum((1, 2)), ab(o[..., 1] * g_dy).sum((1, 2))
        gbox[:, 6], gbox[:, 7] = (ab(gbx * dx) + ab(gby * dy)).sum((1, 2)), sub(ab(gby * dx), ab(gbx * dy)).sum((1, 2))
        gray = gdoff * sg * (1 - sg) * 2 * d_region / D / 2
        daw = (gattn * qw[:, None, :, None]).sum(2)                                # [Q,heads,P]
        dqw = (gattn * aw[:, :, None, :]).sum((1, 3))                              # [Q,T]
        gsc = aw * sub(daw, (aw * daw).sum(-1, keepdim=True))
        gqu = qw * sub(dqw, (qw * dqw).sum(-1, keepdim=True))
        return dict(grad_value=gv, grad_offsets=goff, grad_ray=gray[None], grad_scale=gsc.reshape(1, Q, heads * P),
                    grad_queue=gqu[None], grad_box=gbox[None], grad_loc=gloc[None], grad_attn=gattn[None])


def gather_magnitudes(value, loc, wgt, gout, hw, f32_coords=False):
    """the scales A of tests/test_backward_f64_gpu.py for the gather half: value / attn: the same sums with |value|, |grad_out|
    (weights are non-negative); loc: (W | H) * wgt * sum_taps sum_c |v_c| |g_c| (taps unweighted)"""
    H, W = hw
    gv, _, gattn = gather_grads(value.abs(), loc, wgt.abs(), gout.abs(), hw, f32_coords)
    g = gout.abs()[:, :, None, None, :]
    tot = 0
    for idx, _, _, _, ok in _taps(loc, H, W, f32_coords):
        tot = tot + (_tap_values(value.abs(), idx, loc.shape[1]) * g).sum(-1) * ok
    return gv, torch.stack([W * wgt.abs() * tot, H * wgt.abs() * tot], dim=-1), gattn


def border_distance(qr, off, ray, td, heads, NP, D, H, W, pc, d_region):
    """qr [1,Q,10], off [1,Q,heads*P*2], ray [1,Q,D], td [1,T] (float64) -> [Q,heads,P]: the distance of the keypoints of point
    (h, p), over its frames and both coordinates (before the clamp), to the nearest clamp bound or pixel-cell border, in map units"""
    loc = chain64(box_table_torch(qr, pc)[0], qr[0, :, 8:10], off[0], ray[0], td[0], heads, NP, D, pc, d_region, clamp=False)
    ds = []
    for c, n in ((0, W), (1, H)):
        u = loc[..., c]
        cell = u * n - 0.5
        d_cell = (cell - torch.round(cell)).abs() / n
        ds.append(torch.minimum(torch.minimum(u.abs(), (u - 1).abs()), d_cell))
    return torch.minimum(ds[0], ds[1]).min(2).values


def nudge_query_feat(mod64, qr, qf, td, hw, d_region, margin, seed=0):
    """query_feat [1,Q,E] (float64) moved a little so that every keypoint of the module keeps ``margin`` (map units) from the clamp
    bounds and the pixel-cell borders -- where float32 and float64 locations would pick different taps and the gradient of the
    bilinear sample jumps.  Random search over small changes of the offsets of the points that are too close, carried back to
    query_feat through the pseudo-inverse of the offset / ray Linears (an exact solution that leaves the ray logits alone)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    H, W = hw
    heads, NP, D, pc = mod64.num_heads, mod64.num_points, mod64.depth_num, mod64.pc_range
    _, Q, _ = qf.shape
    with torch.no_grad():
        off, ray = mod64.sampling_offset(qf), mod64.ray_points_offset(qf)
        delta = torch.zeros(Q, heads, NP * D, 2, dtype=torch.float64)
        for _ in range(200):
            bad = border_distance(qr, off + delta.reshape(1, Q, -1), ray, td, heads, NP, D, H, W, pc, d_region) < 2 * margin
            if not bool(bad.any()):
                break
            delta[bad] = torch.from_numpy(rng.uniform(-0.05, 0.05, (int(bad.sum()), 2)))
        assert not bool(bad.any()), f"{int(bad.sum())} points could not be moved clear"
        wcat = torch.cat([mod64.sampling_offset.weight, mod64.ray_points_offset.weight])
        rhs = torch.cat([delta.reshape(1, Q, -1), torch.zeros(1, Q, D, dtype=torch.float64)], dim=-1)
        return qf + rhs @ torch.linalg.pinv(wcat).t()


# ------------------------------------------------------------------------------------------------- fakes of the two launchers
CALLS = []


def fake_fused(value, hw, query_bbox, offsets, ray_logits, scale_logits, queue_logits, time_diff, num_frames, num_heads,
               num_points, depth_num, pc_range, d_region, debug=False, box_table=None, out=None):
    CALLS.append(("fwd", tuple(value.shape), tuple(hw), tuple(query_bbox.shape), offsets.shape[-1], ray_logits.shape[-1],
                  scale_logits.shape[-1], queue_logits.shape[-1], num_frames, num_heads, num_points, depth_num, float(d_region),
                  box_table is not None, debug, out is not None))
    assert not any(x.requires_grad for x in (value, query_bbox, offsets, ray_logits, scale_logits, queue_logits)) or not torch.is_grad_enabled()
    with torch.no_grad():
        o, _ = core64(value, hw, query_bbox, offsets, ray_logits, scale_logits, queue_logits, time_diff, num_frames, num_heads,
                      num_points, depth_num, pc_range, d_region, box_table)
    return o.to(value.dtype)


def fake_backward(value, hw, query_bbox, offsets, ray_logits, scale_logits, queue_logits, time_diff, grad_out, num_frames,
                  num_heads, num_points, depth_num, pc_range, d_region, box_table=None, grad_offsets=None, grad_ray=None,
                  grad_scale=None, grad_queue=None, debug=False):
    CALLS.append(("bwd", tuple(grad_out.shape), grad_out.is_contiguous(), box_table is not None))
    g = closed_form_bwd(value, hw, query_bbox, offsets, ray_logits, scale_logits, queue_logits, time_diff, grad_out, num_frames,
                        num_heads, num_points, depth_num, pc_range, d_region, box_table)
    dt = value.dtype
    res = []
    for dst, key in ((grad_offsets, "grad_offsets"), (grad_ray, "grad_ray"), (grad_scale, "grad_scale"), (grad_queue, "grad_queue")):
        if dst is None:
            dst = torch.empty(g[key].shape, dtype=dt)
        dst.copy_(g[key])
        res.append(dst)
    return (g["grad_value"].to(dt), *res, g["grad_box"].to(dt))
