"""The two-stage float64 criterion for the fused sampling forwards (rac_sampling4d_fwd, rac_bev_sampling_*fwd): cases, references,
bounds and negative controls shared by tests/test_fused_fwd_f64_cpu.py and tests/test_fused_fwd_f64_gpu.py (test helper, no GPU).

The thing under test is a ``runner``: an object with
  table(query_bbox)                       -> the box table [B,Q,8] float32 (the device's rac_box_prep_fwd)
  s4d(c, table, view_in, compact)         -> (out [B,Q,G,T*P,64], loc [S,Q,P,3], w [S,Q,P,L])
  bev(c, table)                           -> (out [B,Q,heads*64], loc [B,Q,heads,T,P,2])
  bev_multi(cs, table)                    -> [out per stream]            (no locations: the launcher has none)
  bev_q16(cs, table)                      -> ([out per stream], [q], [scale])
taking and returning CPU tensors.  ``Restated32`` is the float32 restatement of the same functions on the CPU: it stands in for the
kernels in the CPU module, and gives every comparison its E_ref in the GPU module.

Stage A (keypoints): u, v, the level weights / the BEV locations against the float64 chain on the same float32 inputs, point by
point; cameras equal outside a band of BAND around the discrete gates and among the cameras float64 allows inside it.
Stage B (gather): every element of ``out`` against the float64 gather at the runner's OWN float32 locations, cameras (and, for
sampling4d, level weights): |got - ref| <= bound * 2^-24 * A + TINY, A the same sum with every term non-negative, an element with
A == 0 exactly 0.  bound = max(RATIO * E_ref, 1): E_ref is the float32 restatement's worst err / A on the same case, RATIO the
project's factor for a reordered float32 sum, and 1 the floor of a single rounding."""
import numpy as np
import torch

import bev_sampling_batch_ref as BB
import bev_sampling_ref as BR
import sampling4d_core_ref as SR
from racformer_amd import synthetic as syn
from racformer_amd.transformer import box_table_torch

U = 2.0 ** -24
RATIO = 4.0
TINY = 1e-30
# The band around a gate (image-normalised u, v; ux, uy of the polar grid; homo relative to the magnitude of its four-term sum) has to hold RATIO times the
# float32 chain's own error of the gated quantities: the CPU module asserts BAND >= RATIO * E_ref for every case.
BAND, BAND_CAP = 1e-4, 0.02
IMG = (64, 176)
PC = list(syn.PC_RANGE)
EPS = 1e-5
D_REGION = 0.1
F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------------------- the metric
def figure(got, ref, A):
    """worst |got - ref| / A over the elements with A > 0, in units of 2^-24"""
    got, ref, A = (x.detach().double() for x in (got, ref, A))
    live = A > 0
    if not bool(live.any()):
        return 0.0
    return float(((got - ref).abs()[live] / A[live]).max() / U)


def violations(got, ref, A, bound):
    got, ref, A = (x.detach().double() for x in (got, ref, A))
    return ~((got - ref).abs() <= bound * U * A + TINY)


def bound_of(e_ref):
    return max(RATIO * e_ref, 1.0)


class Log:
    """every (E_ref, kernel) pair of a session; ``check`` prints the pair, then asserts"""

    def __init__(self):
        self.errors = {}

    def check(self, key, e_ref, kernel):
        self.errors[key] = dict(E_ref=e_ref, kernel=kernel)
        print(f"{key}: E_ref {e_ref:.3g}, kernel {kernel:.3g} (allowed {bound_of(e_ref):.3g}) x 2^-24")
        assert kernel <= bound_of(e_ref), f"{key}: {kernel:.3g} above {bound_of(e_ref):.3g} = max({RATIO:g} x E_ref {e_ref:.3g}, 1)"

    def elementwise(self, key, got, ref, A, r32):
        """stage B: every element within the bound, none left out; A == 0 -> exactly 0"""
        assert bool(torch.isfinite(got).all()), f"{key}: non-finite output"
        dead = A == 0
        assert bool((got[dead] == 0).all()), f"{key}: an element without any tap is not 0"
        e_ref = figure(r32, ref, A)
        bad = violations(got, ref, A, bound_of(e_ref))
        self.check(key, e_ref, figure(got, ref, A))
        assert not bool(bad.any())
        return bound_of(e_ref)


def must_fail(key, got, wrong, A, bound):
    assert bool(violations(got, wrong, A, bound).any()), f"negative control {key}: a deliberately wrong reference passed"


# ------------------------------------------------------------------------------------------------------- sampling4d: cases
LEVELS = {2: [(8, 22), (4, 11)], 4: [(8, 22), (4, 11), (2, 6), (1, 3)], 5: [(8, 22), (4, 11), (2, 6), (1, 3), (1, 2)]}


def s4d_rows(P, L, N):
    """queries per workgroup: the launcher's lds_bytes rule (sampling_fused.hip)"""
    rows = 8
    while rows > 1 and (rows * P * 8 * L + N * 16) * 4 + 2 * rows * P > 64 * 1024:
        rows >>= 1
    return rows


def s4d_compact(N, P, compact):
    """whether the launcher takes the COMPACT instantiation"""
    return (N <= 3 if compact is None else bool(compact)) and P <= 64


def s4d_case(seed, B, Q, G, T, NP, D, N, L, three_cam=False, bf16=False, zero_cam=True):
    """float32 inputs of rac_sampling4d_fwd on the ring rig (tests/test_racsampling_grad_cpu.py::_case, every second query beyond
    the polar grid), one draw per batch element; the last camera of the last frame zeroed (homo = 0 <= eps) where the case has
    more than one (frame, camera); offsets / ray / scale logits as column slices of one wider tensor"""
    from test_racsampling_grad_cpu import _case
    hws = LEVELS[L]
    parts = [_case(seed + 101 * b, Q, G, T, NP, D, N, hws, outside=True, three_cam=three_cam)[0] for b in range(B)]
    P = NP * D
    c = dict(B=B, Q=Q, G=G, T=T, NP=NP, D=D, P=P, N=N, L=L, hws=hws, bf16=bf16)
    for k in ("query_bbox", "td", "l2i"):
        c[k] = torch.cat([p[k] for p in parts]).float()
    if zero_cam and T * N > 1:
        c["l2i"][:, T * N - 1] = 0
    feats = [torch.cat([p["feats"][l] for p in parts]).float() for l in range(L)]
    c["feats"] = [f.bfloat16() for f in feats] if bf16 else feats
    widths = (G * P * 3, D, G * T * P * L)
    starts = (3, 3 + widths[0] + 5, 3 + widths[0] + 5 + widths[1])
    wide = torch.randn(B, Q, starts[2] + widths[2] + 1, generator=torch.Generator().manual_seed(seed))
    for k, s0, n in zip(("off", "ray", "sc"), starts, widths):
        wide[..., s0:s0 + n] = torch.cat([p[k] for p in parts]).float()
    c["wide"], c["cols"] = wide, {k: (s0, n) for k, s0, n in zip(("off", "ray", "sc"), starts, widths)}
    s4d_slice(c)
    return c


def s4d_slice(c, wide=None):
    """(re)make the three column slices of ``wide`` (default: the case's own)"""
    wide = c["wide"] if wide is None else wide
    views = {k: wide[..., s0:s0 + n] for k, (s0, n) in c["cols"].items()}
    if wide is c["wide"]:
        c.update(views)
    return views


def kernel_views(loc, N):
    return torch.round(loc[..., 2] * max(N - 1, 1)).long()


def _s4d_chain(c, table, dtype, view=None):
    B, T, G = c["B"], c["T"], c["G"]
    vin = None if view is None else SR.from_slots(view.long(), B, T, G)
    to = lambda x: x.to(dtype)                                                                   # noqa: E731
    return SR.chain64(to(table), to(c["query_bbox"][..., 8:10]), to(c["off"]), to(c["ray"]), to(c["td"]), to(c["l2i"]), G, c["NP"],
                      c["D"], PC, D_REGION, IMG[0], IMG[1], EPS, vin)


def s4d_gather(c, loc, w, cams, dtype=F64, magnitude=False):
    """the gather at given locations [S,Q,P,3], level weights [S,Q,P,L] and cameras [S,Q,P] -> [B,Q,G,T*P,64] in ``dtype``;
    float64 reads the float32 pixel coordinate the kernels form (one float32 product), float32 forms it itself"""
    B, T, G, Q, P = c["B"], c["T"], c["G"], c["Q"], c["P"]
    u, v = (SR.from_slots(loc[..., i].to(dtype), B, T, G) for i in (0, 1))
    smp = SR.sampled64([f.to(dtype) for f in c["feats"]], u, v, SR.from_slots(cams.long(), B, T, G), dtype == F64, magnitude)
    out = (smp * SR.from_slots(w.to(dtype), B, T, G)[..., None]).sum(-2)
    return out.permute(0, 3, 2, 1, 4, 5).reshape(B, Q, G, T * P, 64)


def s4d_geometry(c, table):
    """the float64 chain at its own cameras and every camera's (u, v, homo): the gates, the band around them, the cameras float64
    allows inside the band, and what kinds of points the case holds"""
    B, T, N = c["B"], c["T"], c["N"]
    ch = _s4d_chain(c, table, F64)
    box = table.double()
    sx, sy = PC[3] - PC[0], PC[4] - PC[1]
    X, Y = ch["ux"].clamp(0, 1) * sx + PC[0], ch["uy"].clamp(0, 1) * sy + PC[1]
    pz = (box[..., 2][:, None, :, None] + ch["bh"] * ch["o"][..., 2])[:, None].expand_as(X)
    m = c["l2i"].double().reshape(B, T, N, 16)[:, :, :, None, None, None, :]
    Xc, Yc, Zc = X[:, :, None], Y[:, :, None], pz[:, :, None]
    camx = m[..., 0] * Xc + m[..., 1] * Yc + m[..., 2] * Zc + m[..., 3]
    camy = m[..., 4] * Xc + m[..., 5] * Yc + m[..., 6] * Zc + m[..., 7]
    homo = m[..., 8] * Xc + m[..., 9] * Yc + m[..., 10] * Zc + m[..., 11]
    hz = homo.clamp_min(EPS)
    u, v = camx / hz / IMG[1], camy / hz / IMG[0]                                   # [B,T,N,G,Q,P]
    # (homo's band in units of its own sum's magnitude: a zeroed camera's homo is 0 exactly, in float32 as in float64)
    d = BAND
    hm = BAND * ((m[..., 8] * Xc).abs() + (m[..., 9] * Yc).abs() + (m[..., 10] * Zc).abs() + m[..., 11].abs())
    valid = (homo > EPS) & (v > 0) & (v < 1) & (u > 0) & (u < 1)
    sure = (homo > EPS + hm) & (v > d) & (v < 1 - d) & (u > d) & (u < 1 - d)
    maybe = (homo > EPS - hm) & (v > -d) & (v < 1 + d) & (u > -d) & (u < 1 + d)
    near_clamp = sum(((x.abs() <= d) | ((x - 1).abs() <= d)) for x in (ch["ux"], ch["uy"])) > 0
    band = (sure != maybe).any(2) | near_clamp
    before = torch.cumsum(sure.long(), 2) - sure.long()
    allowed = maybe & (before == 0)
    allowed[:, :, 0] |= ~sure.any(2)
    own = torch.argmax(valid.to(torch.uint8), 2)
    assert torch.equal(own, ch["own"])
    # what the case holds (float64 taps at the chain's own camera)
    part, outside_all = [], True
    for H, W in c["hws"]:
        oks = torch.stack([t[5] for t in SR._taps(ch["u"], ch["v"], H, W, False)])
        part.append(bool((oks.any(0) & ~oks.all(0)).any()))
        outside_all = outside_all & ~oks.any(0)
    holds = dict(in_some_image=bool(valid.any()), no_valid_camera=bool((~valid.any(2)).any()), partial_footprint_on_every_level=all(part),
                 all_taps_outside=bool(outside_all.any()), homo_le_eps=bool((ch["homo"] <= EPS).any()),
                 active_clamp=bool(((ch["ux"] < 0) | (ch["ux"] > 1) | (ch["uy"] < 0) | (ch["uy"] > 1)).any()))
    return dict(chain=ch, u=u, v=v, homo=homo, band=band, allowed=allowed, own=own, holds=holds, share=float(band.float().mean()))


def s4d_gate_error(c, table, geo):
    """the float32 chain's own error of the gated quantities, absolute: u, v of every camera a point is in or near the image of
    (|u|, |v| <= 2, homo > eps), ux, uy near the unit square"""
    B, T, N = c["B"], c["T"], c["N"]
    worst = 0.0
    for n in range(N):
        view = torch.full((B * T * c["G"], c["Q"], c["P"]), n)
        c32, c64 = _s4d_chain(c, table, F32, view), _s4d_chain(c, table, F64, view)
        near = (c64["u"].abs() <= 2) & (c64["v"].abs() <= 2) & (c64["homo"] > EPS)
        for k in ("u", "v"):
            if bool(near.any()):
                worst = max(worst, float((c32[k].double() - c64[k]).abs()[near].max()))
        if n == 0:
            for k in ("ux", "uy"):
                sq = (c64[k] > -1) & (c64[k] < 2)
                worst = max(worst, float((c32[k].double() - c64[k]).abs()[sq].max()))
    return worst


def s4d_check_cameras(c, geo, loc):
    """the runner's own camera choice: float64's outside the band, one of those float64 allows inside it"""
    B, T, G = c["B"], c["T"], c["G"]
    cam = SR.from_slots(kernel_views(loc, c["N"]), B, T, G)
    assert int(cam.min()) >= 0 and int(cam.max()) < c["N"]
    band = geo["band"]
    assert geo["share"] <= BAND_CAP, f"band share {geo['share']:.4f}: a condition on the inputs, not a tolerance -- change the case"
    assert torch.equal(cam[~band], geo["own"][~band]), "a camera differs from float64's outside the band"
    ok = geo["allowed"].gather(2, cam[:, :, None]).squeeze(2)
    assert bool(ok[band].all()), "a band point chose a camera float64 does not allow"
    return int((cam != geo["own"]).sum())


def s4d_stage_a(log, key, c, table, loc, w, view_in=None, plain_slots=False):
    """u, v in the camera the runner sampled in and the level weights, point by point -> the bound of the level weights (for the
    negative control).  u is compared where a tap can depend on it (|u| <= 2: every level is at least 2 wide), v where |v| <= 2 as
    well; the scale of a point is max(1, |ref|)."""
    B, T, G = c["B"], c["T"], c["G"]
    used = kernel_views(loc, c["N"]) if view_in is None else view_in.long()
    c64, c32 = _s4d_chain(c, table, F64, used), _s4d_chain(c, table, F32, used)
    near_u = SR.to_slots(c64["u"].abs() <= 2, B, T, G)
    near_v = near_u & SR.to_slots(c64["v"].abs() <= 2, B, T, G)
    assert bool(near_v.any())
    for i, (k, near) in enumerate((("u", near_u), ("v", near_v))):
        ref = SR.to_slots(c64[k], B, T, G)
        A = ref.abs().clamp_min(1.0) * near
        log.check(f"{key} A {k}", figure(SR.to_slots(c32[k], B, T, G), ref, A), figure(loc[..., i], ref, A))
    w64 = s4d_level_weights(c, F64, plain_slots)
    e_ref = figure(s4d_level_weights(c, F32), s4d_level_weights(c, F64), torch.ones_like(w64))
    if plain_slots:
        return figure(w, w64, torch.ones_like(w64)), bound_of(e_ref)
    log.check(f"{key} A w", e_ref, figure(w, w64, torch.ones_like(w64)))
    assert bool(((w.double().sum(-1) - 1).abs() < 1e-5).all())


def s4d_level_weights(c, dtype, plain_slots=False):
    """[S,Q,P,L]; plain_slots: slot (t, g) reads entry (g, t) of the [G,T] table -- NOT quirk Q1's t*G + g (a wrong reference)"""
    B, T, G, P, L = c["B"], c["T"], c["G"], c["P"], c["L"]
    if not plain_slots:
        return SR.to_slots(SR.level_weights(c["sc"].to(dtype), G, T, P, L), B, T, G)
    w = torch.softmax(c["sc"].to(dtype).reshape(B, c["Q"], G, T, P, L), dim=-1)
    return SR.to_slots(w.permute(0, 3, 2, 1, 4, 5), B, T, G)


def s4d_stage_b(log, key, c, out, loc, w, cams):
    ref, A, r32 = s4d_gather(c, loc, w, cams), s4d_gather(c, loc, w, cams, magnitude=True), s4d_gather(c, loc, w, cams, F32)
    bound = log.elementwise(f"{key} B out", out, ref, A, r32)
    must_fail(f"{key}: one tap dropped", out, s4d_drop_one_tap(c, ref, loc, w, cams), A, bound)
    return ref, A, bound


def s4d_drop_one_tap(c, ref, loc, w, cams):
    """the reference with the top-left tap of one in-range point missing on level 0 (the point of largest weight among them)"""
    B, T, G, P = c["B"], c["T"], c["G"], c["P"]
    H, W = c["hws"][0]
    u, v = (SR.from_slots(loc[..., i].double(), B, T, G) for i in (0, 1))
    hi, wi, tw, _, _, ok = SR._taps(u, v, H, W, True)[0]
    wt = torch.where(ok, tw * SR.from_slots(w[..., 0].double(), B, T, G), torch.zeros_like(tw)).nan_to_num(0.0)
    assert float(wt.max()) > 0, "no in-range point for the negative control"
    b, t, g, q, p = np.unravel_index(int(wt.argmax()), wt.shape)
    s = (b * T + t) * G + g
    wrong = ref.clone()
    wrong[b, q, g, t * P + p] -= float(wt[b, t, g, q, p]) * c["feats"][0][s, int(cams[s, q, p]), int(hi[b, t, g, q, p]), int(wi[b, t, g, q, p])].double()
    return wrong


def check_s4d(log, key, c, runner, compact=None, imposed=False, gate_error=False):
    """stages A and B of one case (and its negative controls) -> what the runner returned"""
    table = runner.table(c["query_bbox"])
    geo = s4d_geometry(c, table)
    print(f"{key}: S={c['B'] * c['T'] * c['G']} Q={c['Q']} P={c['P']} L={c['L']} N={c['N']} rows={s4d_rows(c['P'], c['L'], c['N'])} "
          f"compact={s4d_compact(c['N'], c['P'], compact)} band share {100 * geo['share']:.2f} % holds {geo['holds']}")
    # (the only query of a one-query case is the one beyond the polar grid: its keypoints sit on the grid's border, 50 m from the
    #  rig, inside every image's height -- no footprint of it is cut by an image border)
    need = [k for k in geo["holds"] if c["Q"] > 1 or k != "partial_footprint_on_every_level"]
    assert all(geo["holds"][k] for k in need), geo["holds"]
    if gate_error:
        e = s4d_gate_error(c, table, geo)
        print(f"{key}: float32 error of the gated quantities {e:.3g} (band {BAND:g})")
        assert RATIO * e <= BAND
    out, loc, w = runner.s4d(c, table, None, compact)
    flips = s4d_check_cameras(c, geo, loc)
    print(f"{key}: {flips} cameras differ from float64 (all inside the band)")
    s4d_stage_a(log, key, c, table, loc, w)
    own = kernel_views(loc, c["N"])
    s4d_stage_b(log, key, c, out, loc, w, own)
    if imposed:
        vin = ((own + 1) % c["N"]).to(torch.uint8).contiguous()
        out2, loc2, w2 = runner.s4d(c, table, vin, compact)
        assert torch.equal(loc2[..., 2], loc[..., 2]) and torch.equal(w2, w)         # its own choice is still reported
        assert c["N"] == 1 or not torch.equal(loc2[..., :2], loc[..., :2])
        s4d_stage_a(log, key + " imposed", c, table, loc2, w2, view_in=vin)
        s4d_stage_b(log, key + " imposed", c, out2, loc2, w2, vin)
    return out, loc, w


def s4d_poison(c, q):
    """NaN / inf into the offsets and scale logits of query ``q`` (in place, through the wide tensor's slices)"""
    c["off"][:, q, 0::7] = float("nan")
    c["off"][:, q, 3::7] = float("inf")
    c["off"][:, q, 5::7] = float("-inf")
    c["sc"][:, q, 0::5] = float("nan")
    c["sc"][:, q, 2::5] = float("inf")


# ------------------------------------------------------------------------------------------------------------ BEV: cases
def bev_list_holes(T, P, i16=False):
    """the launcher's list_holes rule (bev_fused.hip)"""
    if i16:
        return ((T * P + 7) // 8 + 3) // 4 * 4 * 8 != T * P
    npp = (P + 3) // 4
    return P % 4 != 0 or (T * npp + 3) // 4 * 4 != T * npp


def bev_case(seed, B, T, Q, heads, NP, D, H, W, bf16=False):
    """float32 inputs of rac_bev_sampling_fwd (tests/test_bev_sampling_batch_grad_cpu.py::case, every second query beyond the map)"""
    from test_bev_sampling_batch_grad_cpu import case
    c, _ = case(seed, B, T, Q, heads, NP, D, H, W, outside=True, dtype=np.float32)
    c.update(B=B, Q=Q, P=NP * D, bf16=bf16)
    if bf16:
        c["value"] = c["value"].bfloat16()
    return c


def bev_second_stream(c, seed, octaves=False):
    """another stream for the same queries: its own values and Linear outputs"""
    H, W = c["hw"]
    c2 = bev_case(seed, c["B"], c["T"], c["Q"], c["heads"], c["NP"], c["D"], H, W, c["bf16"])
    c2["query_bbox"], c2["time_diff"] = c["query_bbox"], c["time_diff"]
    if octaves:
        bev_octaves(c2, seed)
    return c2


def bev_octaves(c, seed):
    """the (pixel, head) blocks of the value stream spread over 2^-12 .. 2^12, one frame's first blocks all zero"""
    g = torch.Generator().manual_seed(seed)
    v = c["value"].float()
    v = v * torch.exp2(torch.randint(-12, 13, v.shape[:-1], generator=g).float())[..., None]
    v[0, :2] = 0
    c["value"] = v


def quantize_i16_cpu(value):
    """int16 block storage on the CPU (the stand-in's; the references read whatever (q, scale) a runner returns): one
    power-of-two scale per block of 64, value ~ q * scale"""
    amax = value.abs().amax(-1)
    scale = torch.where(amax > 0, torch.exp2(torch.floor(torch.log2(amax.clamp_min(1e-37))) - 14), torch.ones_like(amax))
    q = torch.round(value / scale[..., None]).clamp(-32767, 32767).to(torch.int16)
    return q, scale


def bev_chain(c, table, dtype, paired=True):
    """loc [B,Q,heads,T,P,2] by output slot.  B == 1: from the box table, as the kernel; B > 1: the kernel forms every paired
    sample's chain from the query box itself, so the table is box_table_torch's in ``dtype``"""
    B, T, heads, NP, D = c["B"], c["T"], c["heads"], c["NP"], c["D"]
    qb = c["query_bbox"].to(dtype)
    if B == 1:
        return BR.chain64(table[0].to(dtype), qb[0, :, 8:10], c["off"][0].to(dtype), c["ray"][0].to(dtype), c["time_diff"][0].to(dtype),
                          heads, NP, D, PC, D_REGION, dtype=dtype)[None]
    loc_s = BB.chain64_batch(box_table_torch(qb, PC), qb[..., 8:10], c["off"].to(dtype), c["ray"].to(dtype), c["time_diff"].to(dtype),
                             heads, NP, D, PC, D_REGION)
    _, _, b_l, t_l = BB.pairing(B, T, paired)
    return BB._rows(loc_s, b_l, t_l).reshape(c["Q"], heads, B, T, c["P"], 2).permute(2, 0, 1, 3, 4, 5)


def bev_gather(c, loc, dtype=F64, magnitude=False, paired=True, value=None):
    """the gather at given locations [B,Q,heads,T,P,2] with the softmaxes of the logits in ``dtype`` -> [B,Q,heads*64]: row
    r = b_o*T + t_o of the value frames under the point weights of sample b_l = r % B (tests/bev_sampling_batch_ref.py)"""
    B, T, Q, heads, P = c["B"], c["T"], c["Q"], c["heads"], c["P"]
    b_o, t_o, b_l, _ = BB.pairing(B, T, paired)
    loc_r = loc.to(dtype).permute(1, 2, 0, 3, 4, 5).reshape(Q, heads, B * T, P, 2)
    aw = torch.softmax(c["sc"].to(dtype).reshape(B, Q, heads, P), dim=-1)
    qw = torch.softmax(c["qu"].to(dtype), dim=-1)
    wgt = aw[b_l].movedim(0, 2) * qw[b_o, :, t_o].t()[:, None, :, None]
    value = (c["value"] if value is None else value).to(dtype)
    smp = BR.sampled64(value, loc_r, c["hw"], dtype == F64, magnitude)
    rows = (smp * wgt[..., None]).sum(3)
    return rows.reshape(Q, heads, B, T, 64).sum(3).permute(2, 0, 1, 3).reshape(B, Q, heads * 64)


def bev_drop_one_tap(c, ref, loc, value=None):
    """the reference with the heaviest tap of one in-range keypoint of output sample 0 missing"""
    B, T, Q, heads, P = c["B"], c["T"], c["Q"], c["heads"], c["P"]
    H, W = c["hw"]
    b_l = BB.pairing(B, T)[2]
    aw = torch.softmax(c["sc"].double().reshape(B, Q, heads, P), -1)
    qw = torch.softmax(c["qu"].double(), -1)
    best = None
    for idx, tw, _, _, ok in BR._taps(loc.double()[0], H, W, True):                       # [Q,heads,T,P]: rows 0 .. T-1
        wt = torch.where(ok, tw * aw[b_l[:T]].permute(1, 2, 0, 3) * qw[0][:, None, :, None], torch.zeros_like(tw)).nan_to_num(0.0)
        if best is None or float(wt.max()) > float(best[0].max()):
            best = (wt, idx)
    wt, idx = best
    assert float(wt.max()) > 0, "no in-range point for the negative control"
    q, h, t, p = np.unravel_index(int(wt.argmax()), wt.shape)
    value = (c["value"] if value is None else value).double()
    wrong = ref.clone()
    wrong[0, q, h * 64:(h + 1) * 64] -= float(wt[q, h, t, p]) * value[t, int(idx[q, h, t, p]), h]
    return wrong


def bev_stage_a(log, key, c, table, loc):
    ref, r32 = bev_chain(c, table, F64), bev_chain(c, table, F32)
    one = torch.ones_like(ref)
    log.check(f"{key} A loc", figure(r32, ref, one), figure(loc, ref, one))
    assert bool(((loc == 0) | (loc == 1)).any()), "no keypoint on the clamp: half a footprint outside"
    if c["B"] > 1 and c["T"] > 1:
        wrong = bev_chain(c, table, F64, paired=False)
        assert figure(loc, wrong, one) > bound_of(figure(r32, ref, one)), "negative control: the pairing undone passed stage A"


def bev_stage_b(log, key, c, out, loc, value=None, pairing_control=True):
    ref, A, r32 = (bev_gather(c, loc, value=value), bev_gather(c, loc, magnitude=True, value=value),
                   bev_gather(c, loc, F32, value=value))
    bound = log.elementwise(f"{key} B out", out, ref, A, r32)
    must_fail(f"{key}: one tap dropped", out, bev_drop_one_tap(c, ref, loc, value), A, bound)
    if pairing_control and c["B"] > 1 and c["T"] > 1 and c["P"] > 1:             # (T == 1: the pairing is the identity)
        must_fail(f"{key}: the pairing undone", out, bev_gather(c, loc, paired=False, value=value), A, bound)
    return ref, A, bound


def check_bev(log, key, c, runner):
    table = runner.table(c["query_bbox"])
    print(f"{key}: B={c['B']} T={c['T']} Q={c['Q']} heads={c['heads']} P={c['P']} D={c['D']} map {c['hw']} "
          f"list_holes={bev_list_holes(c['T'], c['P'])} ragged={c['Q'] * c['heads'] % 4 != 0}")
    out, loc = runner.bev(c, table)
    bev_stage_a(log, key, c, table, loc)
    bev_stage_b(log, key, c, out, loc)
    return out, loc, table


def bev_poison(c, q):
    c["off"][:, q, 0::7] = float("nan")
    c["off"][:, q, 3::7] = float("inf")
    c["sc"][:, q, 0::5] = float("nan")
    c["sc"][:, q, 2::5] = float("inf")


def check_box_table(log, key, query_bbox, runner):
    """rac_box_prep_fwd against box_table_torch in float64, element by element (scale max(1, |ref|))"""
    t64 = box_table_torch(query_bbox.double(), PC)
    A = t64.abs().clamp_min(1.0)
    log.check(f"{key} box table", figure(box_table_torch(query_bbox.float(), PC), t64, A), figure(runner.table(query_bbox), t64, A))


# ------------------------------------------------------------------------------------------------ the float32 restatement
class Restated32:
    """the same functions in float32 on the CPU: the stand-in for the kernels, and every comparison's E_ref"""

    def table(self, query_bbox):
        return box_table_torch(query_bbox.float(), PC)

    def s4d(self, c, table, view_in=None, compact=None):
        B, T, G, Q, P = c["B"], c["T"], c["G"], c["Q"], c["P"]
        ch = _s4d_chain(c, table, F32, view_in)
        loc = SR.to_slots(torch.stack([ch["u"], ch["v"], ch["own"].float() / max(c["N"] - 1, 1)], -1), B, T, G)
        w = s4d_level_weights(c, F32)
        return s4d_gather(c, loc, w, SR.to_slots(ch["view"], B, T, G), F32), loc, w

    def bev(self, c, table, value=None):
        loc = bev_chain(c, table, F32)
        return bev_gather(c, loc, F32, value=value), loc

    def bev_multi(self, cs, table):
        return [self.bev(c, table)[0] for c in cs]

    def bev_q16(self, cs, table):
        qs, scales = zip(*(quantize_i16_cpu(c["value"].float()) for c in cs))
        return [self.bev(c, table, q.float() * s[..., None])[0] for c, q, s in zip(cs, qs, scales)], list(qs), list(scales)


# ------------------------------------------------------------------------------------------------------------ case tables
# name -> (seed, B, Q, G, T, NP, D, N, L, three_cam, bf16, compact).  The seeds are the first (from an arbitrary start, in steps of
# 7) whose float64 chain alone meets the conditions on the inputs: the band cap, the band holding RATIO x the float32 error of
# the gated quantities, and every kind of point of ``s4d_geometry``'s ``holds``.
S4D_CASES = {}
for _L, _s3, _s6 in ((2, 42, 52), (4, 44, 54), (5, 66, 90)):
    for _bf in (False, True):
        _dt = "bf16" if _bf else "f32"
        S4D_CASES[f"L{_L} {_dt} 3cam"] = (_s3, 1, 9, 2, 2, 2, 3, 3, _L, True, _bf, True)
        S4D_CASES[f"L{_L} {_dt} 6cam"] = (_s6, 1, 9, 2, 2, 2, 3, 6, _L, False, _bf, True)
for _q, _s in ((1, 2455), (7, 67), (9, 111), (19, 79)):
    S4D_CASES[f"rows8 Q{_q}"] = (_s, 1, _q, 1, 3, 4, 3, 6, 4, False, False, None)                # P = 12, S = 3
for _q, _s in ((3, 73), (5, 82), (11, 81)):
    S4D_CASES[f"rows4 Q{_q}"] = (_s, 1, _q, 1, 3, 4, 16, 3, 4, True, False, None)                # P = 64
for _q, _s in ((1, 690), (3, 139), (7, 101)):
    S4D_CASES[f"rows2 Q{_q}"] = (_s, 1, _q, 3, 1, 8, 16, 3, 5, True, False, True)                # P = 128: COMPACT asked, plain taken
S4D_CASES["S9 odd GT"] = (91, 1, 9, 3, 3, 2, 3, 3, 2, True, False, None)
S4D_CASES["S12 B2"] = (99, 2, 9, 3, 2, 2, 3, 6, 4, False, False, None)
S4D_CASES["S16 B2"] = (107, 2, 5, 2, 4, 2, 3, 3, 4, True, False, None)
S4D_CASES["N1"] = (94, 1, 9, 2, 2, 2, 3, 1, 4, False, False, None)
S4D_IMPOSED = ("L4 f32 3cam", "S12 B2")
S4D_ROWS = {"rows8": 8, "rows4": 4, "rows2": 2}


def s4d_build(name):
    seed, B, Q, G, T, NP, D, N, L, three_cam, bf16, compact = S4D_CASES[name]
    return s4d_case(seed, B, Q, G, T, NP, D, N, L, three_cam, bf16), compact


# name -> (seed, T, Q, heads, NP, D, H, W); every one at B in {1, 2} and in f32 / bf16
BEV_SHAPES = {"P20 T8 h4 16x16": (120, 8, 5, 4, 4, 5, 16, 16),
              "P6 T3 h3 5x7": (121, 3, 3, 3, 6, 1, 5, 7),
              "P1 T1 h1 1x9": (122, 1, 5, 1, 1, 1, 1, 9),
              "P32 T3 h4 16x16": (123, 3, 3, 4, 2, 16, 16, 16),
              "P32 T1 h1 5x7": (124, 1, 6, 1, 2, 16, 5, 7),
              "P6 T1 h3 1x9": (125, 1, 3, 3, 6, 1, 1, 9)}
BEV_HOLES = {"P20 T8 h4 16x16": False, "P6 T3 h3 5x7": True, "P1 T1 h1 1x9": True, "P32 T3 h4 16x16": False, "P32 T1 h1 5x7": False,
             "P6 T1 h3 1x9": True}


# the first draw (at B = 1, B = 2) with a keypoint on the clamp: with D = 1 the only depth base pulls every keypoint 6.5 m inwards
BEV_DRAW = {"P20 T8 h4 16x16": (0, 0), "P6 T3 h3 5x7": (15, 3), "P1 T1 h1 1x9": (119, 22), "P32 T3 h4 16x16": (0, 0),
            "P32 T1 h1 5x7": (0, 0), "P6 T1 h3 1x9": (31, 38)}


def bev_build(name, B, bf16=False):
    seed, T, Q, heads, NP, D, H, W = BEV_SHAPES[name]
    return bev_case(seed + 7 * B + 1000 * BEV_DRAW[name][B - 1], B, T, Q, heads, NP, D, H, W, bf16)
