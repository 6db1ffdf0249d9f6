"""float64 torch restatements around rac_sampling4d_fwd / rac_sampling4d_bwd (test helper, no GPU).  Per-keypoint tensors are
[B,T,G,Q,P] (reshaped to the kernels' [S,Q,P] with S = (b*T + t)*G + g); feature levels [S,N,H,W,64] channel-last.

  chain64          the kernel's keypoint chain from the box table on, differentiable: per keypoint (u, v) in the selected camera,
                   the camera, the level weights in the slot order of quirk Q1, and the intermediates the closed form needs
  core64           the whole forward (chain + camera choice + bilinear gather over levels) -> out [B,Q,G,T*P,64]
  gather_grads     the gather half of the backward in closed form at given locations (what rac_msmv_bwd computes per keypoint)
  tail64           the chain tail and the sums in closed form from per-keypoint d/d(u, v) and d/d wl
  closed_form_bwd  the backward the kernel implements, formula by formula (no autograd): every output of its table
  torch_route      the differentiable route the module had before rac_sampling4d_bwd (torch keypoint chain + sampling_4d)
  box_to_query     grad_box -> the gradient of query_ray through box_table_torch (or its magnitude sum)
  gate_margin      how far every keypoint of a chain stays from the discrete gates (clamps, homo > eps)
  fake_fused / fake_backward   drop-in fakes of the two launchers of racformer_amd.fused for CPU plumbing tests
``magnitude=True`` anywhere: the same sums with every term made non-negative -- the scale A of the error metric
worst |err| / A in units of 2^-24.
"""
import math

import torch

from racformer_amd import transformer as _T
from racformer_amd.bbox_utils import theta_d2xy_coods
from racformer_amd.transformer import box_table_torch

TWO_PI = 2 * math.pi


def _f64(x):
    return x.detach().double()


def depth_base(d_region, D):
    return torch.linspace(-d_region, d_region, D).double()     # (formed in float32 as the launcher forms it)


def to_slots(x, B, T, G):
    """[B,T,G,Q,P,...] -> [S,Q,P,...]"""
    return x.reshape(B * T * G, *x.shape[3:])


def from_slots(x, B, T, G):
    return x.reshape(B, T, G, *x.shape[1:])


def grad_out_per_keypoint(gout, T):
    """[B,Q,G,T*P,64] -> [B,T,G,Q,P,64]"""
    B, Q, G, TP, C = gout.shape
    return gout.reshape(B, Q, G, T, TP // T, C).permute(0, 3, 2, 1, 4, 5)


def level_weights(sc, G, T, P, L):
    """scale logits [B,Q,G*T*P*L] -> softmaxed weights per keypoint [B,T,G,Q,P,L]: slot (t, g) reads the (g', t') entry of the
    [G,T] table at flat index t*G + g (sparsebev_sampling.py:113-120, quirk Q1)"""
    B, Q = sc.shape[:2]
    w = torch.softmax(sc.reshape(B, Q, G, T, P, L), dim=-1)
    return w.permute(0, 2, 3, 1, 4, 5).reshape(B, T, G, Q, P, L)


def level_weight_grads_to_logits(g, G, T):
    """the inverse map for gradients: [B,T,G,Q,P,L] -> [B,Q,G*T*P*L]"""
    B, _, _, Q, P, L = g.shape
    return g.reshape(B, G, T, Q, P, L).permute(0, 3, 1, 2, 4, 5).reshape(B, Q, G * T * P * L)


def chain64(box, vel, off, ray, td, l2i, G, NP, D, pc, d_region, image_h, image_w, eps=1e-5, view_in=None):
    """box [B,Q,8], vel [B,Q,2], off [B,Q,G*P*3], ray [B,Q,D], td [B,T], l2i [B,T*N,4,4] (one dtype) -> dict of per-keypoint
    [B,T,G,Q,P] tensors.  ``view_in`` [B,T,G,Q,P] long: the camera to sample in instead of the first valid one."""
    B, Q = box.shape[:2]
    P, T = NP * D, td.shape[1]
    N = l2i.shape[1] // T
    o = off.reshape(B, Q, G, P, 3).permute(0, 2, 1, 3, 4)                   # [B,G,Q,P,3]

    def bx(i):
        return box[..., i][:, None, :, None]                                 # [B,1,Q,1]
    dx, dy, dz = bx(3) * o[..., 0], bx(4) * o[..., 1], bx(5) * o[..., 2]
    cs, sn = bx(6), bx(7)
    bpx, bpy, bpz = bx(0) + (dx * cs - dy * sn), bx(1) + (dx * sn + dy * cs), bx(2) + dz      # [B,G,Q,P]
    tdd = td[:, :, None, None, None]
    px = bpx[:, None] - vel[..., 0][:, None, None, :, None] * tdd             # [B,T,G,Q,P]
    py = bpy[:, None] - vel[..., 1][:, None, None, :, None] * tdd
    pz = bpz[:, None].expand_as(px)
    sx, sy = pc[3] - pc[0], pc[4] - pc[1]
    ex, ey = (px - pc[0]) / sx * 102.4 - 51.2, (py - pc[1]) / sy * 102.4 - 51.2
    sg = torch.sigmoid(ray)
    doff = depth_base(d_region, D).to(ray) + (sg * 2 - 1) * d_region / D / 2  # [B,Q,D]
    doff = doff.repeat(1, 1, NP)[:, None, None]                               # p % D
    r2 = ex * ex + ey * ey
    r = torch.sqrt(r2)
    ang = torch.remainder(torch.atan2(ey, ex) + TWO_PI, TWO_PI)
    rad = (r / 65.0 + doff) * 65.0
    ca, sa = torch.cos(ang), torch.sin(ang)
    ux, uy = (51.2 + rad * ca) / 102.4, (51.2 + rad * sa) / 102.4
    X, Y = ux.clamp(0, 1) * sx + pc[0], uy.clamp(0, 1) * sy + pc[1]
    m = l2i.reshape(B, T, N, 16)

    def project(mm, Xc, Yc, Zc):
        camx = mm[..., 0] * Xc + mm[..., 1] * Yc + mm[..., 2] * Zc + mm[..., 3]
        camy = mm[..., 4] * Xc + mm[..., 5] * Yc + mm[..., 6] * Zc + mm[..., 7]
        homo = mm[..., 8] * Xc + mm[..., 9] * Yc + mm[..., 10] * Zc + mm[..., 11]
        hz = torch.where(homo > eps, homo, torch.full_like(homo, eps))        # (torch.maximum: gradient where homo > eps)
        return camx, camy, homo, hz, camx / hz / image_w, camy / hz / image_h
    with torch.no_grad():
        _, _, homo_a, _, u_a, v_a = project(m[:, :, :, None, None, None, :], X[:, :, None], Y[:, :, None], pz[:, :, None])
        valid = (homo_a > eps) & (v_a > 0) & (v_a < 1) & (u_a > 0) & (u_a < 1)   # [B,T,N,G,Q,P]
        own = torch.argmax(valid.to(torch.uint8), dim=2)                          # first valid / 0
    view = own if view_in is None else view_in
    b_i = torch.arange(B, device=box.device)[:, None, None, None, None]
    t_i = torch.arange(T, device=box.device)[None, :, None, None, None]
    msel = m[b_i, t_i, view]                                                  # [B,T,G,Q,P,16]
    camx, camy, homo, hz, u, v = project(msel, X, Y, pz)
    return dict(u=u, v=v, view=view, own=own, any_valid=valid.any(2), msel=msel, camx=camx, camy=camy, homo=homo, hz=hz, ux=ux, uy=uy, rad=rad,
                ca=ca, sa=sa, ex=ex, ey=ey, r=r, r2=r2, sg=sg, o=o, dx=dx, dy=dy, cs=cs, sn=sn, bw=bx(3), bl=bx(4), bh=bx(5), N=N, T=T)


def _taps(u, v, H, W, f32_coords):
    """-> list of (row, column, weight, d weight / d h_im, d weight / d w_im, ok) with the msmv semantics (align_corners=True)"""
    if f32_coords:     # the pixel coordinate as the kernels form it: one float32 product
        h_im = (v.float() * float(H - 1)).double() + (v - v.detach()) * (H - 1)
        w_im = (u.float() * float(W - 1)).double() + (u - u.detach()) * (W - 1)
    else:
        h_im, w_im = v * (H - 1), u * (W - 1)
    guard = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
    hs, ws = torch.where(guard, h_im, torch.zeros_like(h_im)), torch.where(guard, w_im, torch.zeros_like(w_im))
    hl, wl = torch.floor(hs.detach()), torch.floor(ws.detach())
    lh, lw = hs - hl, ws - wl
    hh, hw = 1 - lh, 1 - lw
    out = []
    for a, b, tw, dh, dw in ((0, 0, hh * hw, -hw, -hh), (0, 1, hh * lw, -lw, hh), (1, 0, lh * hw, hw, -lh), (1, 1, lh * lw, lw, lh)):
        hi, wi = hl.long() + a, wl.long() + b
        ok = guard & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
        out.append((hi.clamp(0, H - 1), wi.clamp(0, W - 1), tw, dh, dw, ok))
    return out


def floors(u, v, hws):
    """the tap cell of every keypoint in every level, [.., L, 2] long (and the guard): what float32 and float64 must agree on"""
    res = []
    for H, W in hws:
        h_im, w_im = v * (H - 1), u * (W - 1)
        guard = (h_im > -1) & (w_im > -1) & (h_im < H) & (w_im < W)
        res.append(torch.stack([torch.where(guard, torch.floor(h_im), torch.full_like(h_im, -9)),
                                torch.where(guard, torch.floor(w_im), torch.full_like(w_im, -9))], -1).long())
    return torch.stack(res, -2)


def sampled64(feats, u, v, view, f32_coords=False, magnitude=False):
    """bilinear(feat_l[s][view], (u, v)) per level -> [B,T,G,Q,P,L,64], differentiable in feats, u, v.  magnitude: |feat| under
    |tap weight|, the scale A of a forward's error bound"""
    B, T, G, Q, P = u.shape
    if magnitude:
        feats = [f.abs() for f in feats]
    s_i = torch.arange(B * T * G, device=u.device).reshape(B, T, G, 1, 1).expand_as(u)
    res = []
    for f in feats:
        H, W = f.shape[2:4]
        s = 0
        for hi, wi, tw, _, _, ok in _taps(u, v, H, W, f32_coords):
            s = s + f[s_i, view, hi, wi] * ((tw.abs() if magnitude else tw) * ok)[..., None]
        res.append(s)
    return torch.stack(res, dim=-2)


def core64(feats, query_bbox, off, ray, sc, td, l2i, T, G, NP, D, pc, d_region, image_h, image_w, eps=1e-5, box_table=None,
           view_in=None, f32_coords=False):
    """float64 forward of rac_sampling4d_fwd -> (out [B,Q,G,T*P,64], chain dict).  ``view_in`` u8 [S,Q,P] as the launcher takes it."""
    B, Q = query_bbox.shape[:2]
    P, L = NP * D, len(feats)
    qb = query_bbox.double()
    box = box_table_torch(qb, pc) if box_table is None else box_table.double()
    vin = None if view_in is None else from_slots(view_in.long(), B, T, G)
    c = chain64(box, qb[..., 8:10].detach(), off.double(), ray.double(), td.double(), l2i.double(), G, NP, D, pc, d_region,
                image_h, image_w, eps, vin)
    wl = level_weights(sc.double(), G, T, P, L)
    smp = sampled64([f.double() for f in feats], c["u"], c["v"], c["view"], f32_coords)   # [B,T,G,Q,P,L,64]
    out = (smp * wl[..., None]).sum(-2)                                                    # [B,T,G,Q,P,64]
    c["wl"] = wl
    return out.permute(0, 3, 2, 1, 4, 5).reshape(B, Q, G, T * P, 64), c


def gather_grads(feats, u, v, view, wl, g, f32_coords=False, magnitude=False):
    """feats[l] [S,N,H,W,64], u, v, view [B,T,G,Q,P], wl [B,T,G,Q,P,L], g [B,T,G,Q,P,64] (float64) ->
    grad_feats (list), grad_u, grad_v [B,T,G,Q,P], grad_wl [B,T,G,Q,P,L]: the closed form of rac_msmv_bwd per keypoint.
    magnitude: |feat|, |g|, and for the locations the taps unweighted ((W-1 | H-1) * wl * sum_taps sum_c |f_c| |g_c|)."""
    B, T, G, Q, P = u.shape
    s_i = torch.arange(B * T * G, device=u.device).reshape(B, T, G, 1, 1).expand_as(u)
    if magnitude:
        feats, g = [f.abs() for f in feats], g.abs()
    gfs, gu, gv, gw = [], 0, 0, []
    for l, f in enumerate(feats):
        H, W = f.shape[2:4]
        gf = torch.zeros_like(f)
        sv, sh, sw = 0, 0, 0
        for hi, wi, tw, dh, dw, ok in _taps(u, v, H, W, f32_coords):
            val = f[s_i, view, hi, wi] * ok[..., None]
            dot = (val * g).sum(-1)
            if magnitude:
                dh = dw = torch.ones_like(tw)
            sv, sh, sw = sv + tw * dot, sh + dh * dot, sw + dw * dot
            gf.index_put_((s_i, view, hi, wi), (tw * wl[..., l] * ok)[..., None] * g, accumulate=True)
        gfs.append(gf)
        gw.append(sv)
        gu, gv = gu + (W - 1) * sw * wl[..., l], gv + (H - 1) * sh * wl[..., l]
    return gfs, gu, gv, torch.stack(gw, -1)


def tail64(c, wl, gu, gv, gwl, G, NP, D, pc, d_region, image_h, image_w, eps=1e-5, magnitude=False, wrong_term=False):
    """The chain tail and the sums of rac_sampling4d_bwd in closed form.  c: chain64's dict (float64), wl [B,T,G,Q,P,L], and per
    keypoint d/d u, d/d v, d/d wl -> dict(grad_offsets [B,Q,G*P*3], grad_ray [B,Q,D], grad_scale [B,Q,G*T*P*L], grad_box [B,Q,8]).
    ``wrong_term``: the clamp gates left out (a deliberately wrong reference, for the negative control)."""
    ab = (lambda x: x.abs()) if magnitude else (lambda x: x)
    sub = (lambda x, y: x + y) if magnitude else (lambda x, y: x - y)
    m = c["msel"]
    B, T, _, Q, P = gu.shape
    sx, sy = pc[3] - pc[0], pc[4] - pc[1]
    hz = c["hz"]
    g_camx, g_camy = gu / (hz * image_w), gv / (hz * image_h)
    g_homo = torch.where(c["homo"] > eps, (ab(g_camx * c["camx"]) + ab(g_camy * c["camy"])) / hz, torch.zeros_like(hz))
    if not magnitude:
        g_homo = -g_homo
    gX = ab(m[..., 0] * g_camx) + ab(m[..., 4] * g_camy) + ab(m[..., 8] * g_homo)
    gY = ab(m[..., 1] * g_camx) + ab(m[..., 5] * g_camy) + ab(m[..., 9] * g_homo)
    gz = ab(m[..., 2] * g_camx) + ab(m[..., 6] * g_camy) + ab(m[..., 10] * g_homo)
    ux, uy = c["ux"], c["uy"]
    in_x = (ux >= 0) & (ux <= 1) if not wrong_term else torch.ones_like(ux, dtype=torch.bool)
    in_y = (uy >= 0) & (uy <= 1) if not wrong_term else torch.ones_like(uy, dtype=torch.bool)
    gux = torch.where(in_x, gX * sx / 102.4, torch.zeros_like(ux))
    guy = torch.where(in_y, gY * sy / 102.4, torch.zeros_like(uy))
    ca, sa, ex, ey, r, r2 = c["ca"], c["sa"], c["ex"], c["ey"], c["r"], c["r2"]
    g_rad = ab(gux * ca) + ab(guy * sa)
    g_ang = ab(c["rad"]) * sub(ab(guy * ca), ab(gux * sa))
    pos = r2 > 0
    ir, ir2 = torch.where(pos, 1 / r, torch.zeros_like(r)), torch.where(pos, 1 / r2, torch.zeros_like(r))
    gpx = (sub(ab(g_rad * ex * ir), ab(g_ang * ey * ir2)) * 102.4 / sx).sum(1)     # sums over frames: [B,G,Q,P]
    gpy = ((ab(g_rad * ey * ir) + ab(g_ang * ex * ir2)) * 102.4 / sy).sum(1)
    gpz = gz.sum(1)
    gdoff = (g_rad * 65.0).sum((1, 2)).reshape(B, Q, NP, D).sum(2)                 # [B,Q,D]
    cs, sn, o, dx, dy = c["cs"], c["sn"], c["o"], c["dx"], c["dy"]
    g_dx, g_dy = ab(gpx * cs) + ab(gpy * sn), sub(ab(gpy * cs), ab(gpx * sn))
    bw, bl, bh = c["bw"], c["bl"], c["bh"]
    goff = torch.stack([ab(bw * g_dx), ab(bl * g_dy), ab(bh * gpz)], dim=-1)       # [B,G,Q,P,3]
    goff = goff.permute(0, 2, 1, 3, 4).reshape(B, Q, G * P * 3)
    gbox = torch.stack([gpx.sum((1, 3)), gpy.sum((1, 3)), gpz.sum((1, 3)), ab(o[..., 0] * g_dx).sum((1, 3)),
                        ab(o[..., 1] * g_dy).sum((1, 3)), ab(o[..., 2] * gpz).sum((1, 3)),
                        (ab(gpx * dx) + ab(gpy * dy)).sum((1, 3)), sub(ab(gpy * dx), ab(gpx * dy)).sum((1, 3))], dim=-1)
    sg = c["sg"]
    gray = gdoff * sg * (1 - sg) * 2 * d_region / D / 2
    gl = wl * sub(ab(gwl), (wl * ab(gwl)).sum(-1, keepdim=True))
    return dict(grad_offsets=goff, grad_ray=gray, grad_scale=level_weight_grads_to_logits(gl, G, T), grad_box=gbox)


def closed_form_bwd(feats, query_bbox, off, ray, sc, td, l2i, gout, T, G, NP, D, pc, d_region, image_h, image_w, eps=1e-5,
                    box_table=None, view_in=None, f32_coords=False, loc_at=None, magnitude=False, wrong_term=False, given=None):
    """The backward rac_sampling4d_bwd implements, in float64 without autograd -> dict(grad_feats (list), grad_offsets,
    grad_ray, grad_scale, grad_box, grad_u, grad_v, grad_wl (per keypoint, [B,T,G,Q,P(,L)])).
    ``view_in`` u8 [S,Q,P]: imposed cameras.  ``loc_at`` (u, v) [S,Q,P] each: gather at these locations (a forward's own
    loc_out) instead of the float64 chain's, so that the taps are that forward's; the chain tail stays the float64 Jacobian.
    ``given`` (grad_u, grad_v, grad_wl): per-keypoint gradients to feed the tail instead of the gather half's own."""
    with torch.no_grad():
        B, Q = query_bbox.shape[:2]
        P, L = NP * D, len(feats)
        qb = _f64(query_bbox)
        box = box_table_torch(qb, pc) if box_table is None else _f64(box_table)
        vin = None if view_in is None else from_slots(view_in.long().to(query_bbox.device), B, T, G)
        c = chain64(box, qb[..., 8:10], _f64(off), _f64(ray), _f64(td), _f64(l2i), G, NP, D, pc, d_region, image_h, image_w, eps, vin)
        wl = level_weights(_f64(sc), G, T, P, L)
        u, v = (c["u"], c["v"]) if loc_at is None else (from_slots(_f64(x), B, T, G) for x in loc_at)
        g = grad_out_per_keypoint(_f64(gout), T)
        gfs, gu, gv, gwl = gather_grads([_f64(f) for f in feats], u, v, c["view"], wl, g, f32_coords, magnitude)
        if given is not None:
            gu, gv, gwl = (_f64(x) for x in given)
            if magnitude:
                gu, gv, gwl = gu.abs(), gv.abs(), gwl.abs()
        res = tail64(c, wl, gu, gv, gwl, G, NP, D, pc, d_region, image_h, image_w, eps, magnitude, wrong_term)
        res.update(grad_feats=gfs, grad_u=gu, grad_v=gv, grad_wl=gwl, chain=c)
        return res


def metric(got, want, scale):
    """worst |got - want| / A in units of 2^-24, A = max(scale, a floor that keeps empty sums out)"""
    got, want, scale = (x.detach().cpu().double() for x in (got, want, scale))
    a = scale.clamp_min(1e-30)
    live = scale > 0
    if not bool(live.any()):
        return 0.0
    return float((((got - want).abs() / a)[live]).max() * 2 ** 24)


def torch_route(qr, off, ray, sc, feats, td, l2i, T, G, NP, D, L, pc, d_region, image_h, image_w, view_in=None):
    """What gave RaCFormerSampling's gradients before rac_sampling4d_bwd: the module's torch helpers for the keypoint chain
    (make_sample_points, _warp_to_polar, theta_d2xy_coods) and the differentiable sampling_4d (rac_msmv_fwd / rac_msmv_bwd_ex),
    in the dtype of its inputs -> [B,Q,G,T*P,64].  ``view_in`` u8 [S,Q,P]: imposed cameras."""
    B, Q, _ = qr.shape
    pts = _T.make_sample_points(theta_d2xy_coods(qr), off.reshape(B, Q, G * NP * D, 3), pc).view(B, Q, 1, G, NP * D, 3)
    theta, dist = _T._warp_to_polar(pts[..., 0:2], qr[..., 8:].detach(), td, pc)
    base = torch.linspace(-d_region, d_region, D, device=qr.device)
    d_off = base + (torch.sigmoid(ray) * 2 - 1) * d_region / D / 2
    dist = (dist.view(B, Q, T, G, NP, D) + d_off[:, :, None, None, None, :]).reshape(B, Q, T, G, NP * D, 1)
    xy = theta_d2xy_coods(torch.cat([theta, dist], dim=-1))
    p3 = torch.cat([xy[..., 0:1] * (pc[3] - pc[0]) + pc[0], xy[..., 1:2] * (pc[4] - pc[1]) + pc[1],
                    pts[..., 2:3].expand(B, Q, T, G, NP * D, 1)], dim=-1)
    sw = torch.softmax(sc.view(B, Q, G, T, NP * D, L), dim=-1)
    return _T.sampling_4d(p3, feats, sw, l2i, image_h, image_w, view_in=view_in)


def box_to_query(query_bbox, pc, grad_box, magnitude=False):
    """grad_box [B,Q,8] -> the gradient of query_bbox [B,Q,10] through box_table_torch, in float64.  magnitude: every term of
    that (per query 8-term) sum non-negative."""
    qb = _f64(query_bbox).requires_grad_()
    table = box_table_torch(qb, pc)
    gb = _f64(grad_box).to(qb.device)
    if not magnitude:
        return torch.autograd.grad(table, qb, gb)[0]
    res = 0
    for i in range(8):
        e = torch.zeros_like(table)
        e[..., i] = 1
        res = res + torch.autograd.grad(table, qb, e, retain_graph=True)[0].abs() * gb[..., i:i + 1].abs()
    return res


def gate_margin(c, eps=1e-5):
    """the smallest distance of a keypoint of chain64's dict ``c`` from a discrete gate of the backward: the two clamps (ux, uy
    at 0 and 1) and homo at eps, the latter relative to |homo| + 1"""
    m = min(float(torch.minimum(x.abs(), (x - 1).abs()).min()) for x in (c["ux"], c["uy"]))
    return min(m, float(((c["homo"] - eps).abs() / (c["homo"].abs() + 1)).min()))


# ------------------------------------------------------------------------------------------------- fakes of the two launchers
CALLS = []


def fake_fused(mlvl_feats, query_bbox, offsets, ray_logits, scale_logits, time_diff, lidar2img, num_frames, num_groups,
               num_points, depth_num, pc_range, d_region, image_h, image_w, eps=1e-5, debug=False, box_table=None, view_in=None,
               compact=None):
    feats = list(mlvl_feats)
    CALLS.append(("fwd", len(feats), tuple(feats[0].shape), tuple(query_bbox.shape), offsets.shape[-1], ray_logits.shape[-1],
                  scale_logits.shape[-1], num_frames, num_groups, num_points, depth_num, float(d_region), float(image_h),
                  float(image_w), float(eps), debug, box_table is not None, view_in is not None, compact))
    assert not any(x.requires_grad for x in (*feats, query_bbox, offsets, ray_logits, scale_logits)) or not torch.is_grad_enabled()
    with torch.no_grad():
        o, c = core64(feats, query_bbox, offsets, ray_logits, scale_logits, time_diff, lidar2img, num_frames, num_groups,
                      num_points, depth_num, pc_range, d_region, image_h, image_w, eps, box_table, view_in)
    dt = feats[0].dtype
    if not debug:
        return o.to(dt)
    B, T, G = query_bbox.shape[0], num_frames, num_groups
    loc = torch.stack([c["u"], c["v"], c["own"].double() / max(c["N"] - 1, 1)], dim=-1)
    return o.to(dt), to_slots(loc, B, T, G).to(dt), to_slots(c["wl"], B, T, G).to(dt)


def fake_backward(mlvl_feats, query_bbox, offsets, ray_logits, scale_logits, time_diff, lidar2img, grad_out, num_frames,
                  num_groups, num_points, depth_num, pc_range, d_region, image_h, image_w, eps=1e-5, box_table=None, view_in=None,
                  grad_offsets=None, grad_ray=None, grad_scale=None, want_feats=True, debug=False):
    feats = list(mlvl_feats)
    CALLS.append(("bwd", tuple(grad_out.shape), grad_out.is_contiguous(), box_table is not None, view_in is not None, want_feats))
    if any(f.dtype not in (torch.float32, torch.float64) for f in feats):
        raise RuntimeError("sampling4d_backward: float32 features only")
    g = closed_form_bwd(feats, query_bbox, offsets, ray_logits, scale_logits, time_diff, lidar2img, grad_out, num_frames,
                        num_groups, num_points, depth_num, pc_range, d_region, image_h, image_w, eps, box_table, view_in)
    dt = feats[0].dtype
    res = []
    for dst, key in ((grad_offsets, "grad_offsets"), (grad_ray, "grad_ray"), (grad_scale, "grad_scale")):
        if dst is None:
            dst = torch.empty(g[key].shape, dtype=dt)
        dst.copy_(g[key])
        res.append(dst)
    return ([x.to(dt) for x in g["grad_feats"]] if want_feats else None, *res, g["grad_box"].to(dt))
