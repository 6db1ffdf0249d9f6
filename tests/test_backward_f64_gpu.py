"""Every backward kernel path against a float64 reference, element by element, at the shapes and locations where gathers
go wrong: rac_msmv_bwd (C = 64 fast path at L = 2 / 4 / 5, the generic kernel over C, L, N and past its 4096-block grid),
rac_msmv_v2_bwd (C = 64 channel-last, channel-first, past the grid), rac_msda_bwd (d64 over heads and ragged levels with
gaps, the generic kernel over dim and past the grid) and rac_bev_pool_v2_bwd (every lane width, whole and partial, and
the scalar kernel), all through the public autograd entry points.

Reference: the oracle's autograd (oracle/restate.py) in float64, with the sampling coordinates formed in float32 as the
kernels form them (``f32_coords``), so both pick the same taps, guard and camera.

Error bound, per element: ``|got - ref| <= K[kind] * 2**-24 * A + TINY``, where A is a float64 magnitude of the same
gradient with every term made non-negative:
  feat / value / bev feat / bev depth : the oracle backward with |grad_out| and |weights| (|depth|, |feat|);
  w / attn                           : the oracle backward with |features| and |grad_out|;
  loc                                : sum over levels of (W-1 | H-1) * |w| * sum_c |g_c| * sum_taps |v| (W | H for MSDA).
An element whose A is 0 must be exactly 0.  The worst err / A of every gradient kind is printed at the end of the module.

Negative control: every comparison is repeated against a reference with one tap of one point dropped (one point of
one interval for bev_pool), and that comparison must fail for every gradient kind.

Locations include exact integer taps (H-1, W-1 powers of two; MSDA: H, W), 0 and 1, coordinates in (-1, 0), exactly -1
and exactly H (excluded), H - eps (included), 1 x W and H x 1 levels, halfway camera values, and NaN / +-inf (zero
gradients, no NaN written anywhere).
"""
import math

import numpy as np
import pytest
import torch

from oracle import restate as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
# One factor per gradient kind.  Atomic scatters (feat: also bev_pool's feature rows) sum many rounded terms in an
# arbitrary order, up to 100,000 per element here; w / attn / bev depth and loc are one rounded channel sum per element.
# Observed worst on the MI355X, in units of 2**-24: feat 15.3 (the MSDA collision case), w 4.1, loc 4.3.
K = {"feat": 64.0, "w": 16.0, "loc": 16.0}
TINY = 1e-30
WORST = {}
FAR = -4.0   # a finite location outside every map (no level here is 1 x 1): what a NaN / inf location must behave like


@pytest.fixture(scope="module", autouse=True)
def _cpu_threads_and_report():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)
    print("\nworst err/A per gradient kind, in units of 2**-24 (bound K):")
    for name in sorted(WORST):
        kind = name.split(":")[0]
        print(f"  {name:>34s}: {WORST[name] / U:9.3f}   (K = {K[kind]:g})")


def _violations(kind, got, ref, A):
    got, ref, A = got.detach().cpu().double(), ref.detach().cpu().double(), A.detach().cpu().double()
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    err = (got - ref).abs()
    bad = ~(err <= K[kind] * U * A + TINY)          # NaN counts as a violation
    return err, bad


def check(name, kind, got, ref, A):
    """assert the per-element bound; record the worst err / A under `kind:name`"""
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite gradient written"
    err, bad = _violations(kind, got, ref, A)
    A64 = A.detach().cpu().double()
    pos = A64 > 0
    worst = float((err[pos] / A64[pos]).max()) if bool(pos.any()) else 0.0
    key = f"{kind}:{name}"
    WORST[key] = max(WORST.get(key, 0.0), worst)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        pytest.fail(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside {K[kind]:g}*2^-24*A; first at flat {i}: "
                    f"got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} A {float(A64.flatten()[i])!r}")


def must_fail(name, kind, got, wrong, A):
    _, bad = _violations(kind, got, wrong, A)
    assert bool(bad.any()), f"negative control {name}: a reference with one tap dropped passed the {kind} check"


# ------------------------------------------------------------------------------------------------------------- geometry
def _f32c(x, scale, shift=0.0):
    """the kernels' sampling coordinate x * scale - shift, each operation rounded in float32, as float64"""
    y = x.float() * scale
    return (y - shift if shift else y).double()


def _taps(h, w, H, W):
    """float32-formed coordinates h, w [K] -> guard [K] and the four taps (hi, wi, weight, d/dh, d/dw, ok), float64"""
    guard = (h > -1) & (w > -1) & (h < H) & (w < W)
    hs, ws = torch.where(guard, h, torch.zeros_like(h)), torch.where(guard, w, torch.zeros_like(w))
    hl, wl = torch.floor(hs), torch.floor(ws)
    lh, lw = hs - hl, ws - wl
    hh, hw = 1 - lh, 1 - lw
    taps = []
    for a, b, tw, dh, dw in ((0, 0, hh * hw, -hw, -hh), (0, 1, hh * lw, -lw, hh), (1, 0, lh * hw, hw, -lh),
                             (1, 1, lh * lw, lw, lh)):
        hi, wi = hl.long() + a, wl.long() + b
        ok = guard & (hi >= 0) & (hi <= H - 1) & (wi >= 0) & (wi <= W - 1)
        taps.append((hi.clamp(0, H - 1), wi.clamp(0, W - 1), tw, dh, dw, ok))
    return guard, taps


def _finite_for_oracle(loc_uv):
    """the oracle's copy of the locations: a point with a non-finite coordinate moved to (FAR, FAR)"""
    bad = ~torch.isfinite(loc_uv).all(-1, keepdim=True)
    return torch.where(bad, torch.full_like(loc_uv, FAR), loc_uv)


# -------------------------------------------------------------------------------------------------------- msmv / msmv v2
class MsmvGeom:
    """per level: image index, guard and taps of every point (float32 coordinates, the kernels' clamped camera)"""

    def __init__(self, hws, loc, N):
        S, Q, P, _ = loc.shape
        self.K = S * Q * P
        lf = loc.reshape(-1, 3).cpu()
        view = R._round_half_away(_f32c(lf[:, 2], N - 1)).clamp(0, N - 1).long()
        self.img = torch.arange(S).repeat_interleave(Q * P) * N + view
        self.levels = []
        for H, W in hws:
            self.levels.append(_taps(_f32c(lf[:, 1], H - 1), _f32c(lf[:, 0], W - 1), H, W))

    def tap_values(self, feat, l, t):
        """[K, C] float64 values of tap t of level l (0 where the tap is out)"""
        S, N, H, W, C = feat.shape
        hi, wi, _, _, _, ok = self.levels[l][1][t]
        v = feat.detach().cpu().double().reshape(S * N, H, W, C)[self.img, hi, wi]
        return torch.where(ok[:, None], v, torch.zeros_like(v))


def _g_rows(gout):
    """grad_out [S,Q,C,P] -> [S*Q*P, C] float64"""
    S, Q, C, P = gout.shape
    return gout.detach().cpu().double().permute(0, 1, 3, 2).reshape(-1, C)


def msmv_reference(feats, loc, w, gout, N, v2=False):
    """float64 oracle gradients and their magnitudes.  v2: the one-hot identity (the argmax level alone, weight 1), no grad_w.
    -> dict kind -> (ref list, A list) with feat: per level, w: [S,Q,P,L], loc: [S,Q,P,3]"""
    hws = [tuple(f.shape[2:4]) for f in feats]
    L = len(feats)
    loc_c = loc.detach().cpu()
    w_c = w.detach().cpu()
    if v2:
        w_c = torch.nn.functional.one_hot(torch.argmax(w_c, -1), L).float()
    loc_o = torch.cat([_finite_for_oracle(loc_c[..., :2]), loc_c[..., 2:]], -1).double()
    g64 = gout.detach().cpu().double()
    # gradients
    f64 = [f.detach().cpu().double().requires_grad_() for f in feats]
    l64 = loc_o.clone().requires_grad_()
    w64 = w_c.double().requires_grad_(not v2)
    fwd = R.msmv_gather_torch(f64, l64, w64, f32_coords=True)
    fwd.backward(g64)
    # magnitudes of the output and of feat / w
    fa = [f.detach().cpu().double().abs().requires_grad_() for f in feats]
    wa = w_c.double().abs().requires_grad_()
    fwd_a = R.msmv_gather_torch(fa, loc_o, wa, f32_coords=True)
    fwd_a.backward(g64.abs())
    # magnitude of loc
    geo = MsmvGeom(hws, loc_c, N)
    ga = _g_rows(gout).abs()
    wa_rows = w_c.double().abs().reshape(-1, L)
    au = torch.zeros(geo.K, dtype=torch.float64)
    av = torch.zeros_like(au)
    for l, (H, W) in enumerate(hws):
        T = sum((geo.tap_values(feats[l], l, t).abs() * ga).sum(-1) for t in range(4))
        au += (W - 1) * wa_rows[:, l] * T
        av += (H - 1) * wa_rows[:, l] * T
    A_loc = torch.stack([au, av, torch.zeros_like(au)], -1).reshape(loc.shape)
    out = {"feat": ([f.grad for f in f64], [f.grad for f in fa]), "loc": (l64.grad, A_loc),
           "out": (fwd.detach(), fwd_a.detach())}
    if not v2:
        out["w"] = (w64.grad, wa.grad)
    out["geo"], out["w_used"] = geo, w_c.double()
    return out


def msmv_drop_one_tap(ref, feats, gout, hws):
    """the reference with the top-left tap of one in-range point on level 0 dropped (the point of largest tap weight among
    the first in-range ones): -> dict kind -> wrong reference"""
    geo, wu = ref["geo"], ref["w_used"]
    guard, taps = geo.levels[0]
    hi, wi, tw, dh, dw, ok = taps[0]
    l0 = 0
    cand = (ok & (wu.reshape(geo.K, -1)[:, l0] > 0)).nonzero().flatten()
    assert cand.numel() > 0, "no in-range point for the negative control"
    cand = cand[:64]
    k = int(cand[torch.argmax(tw[cand])])
    g = _g_rows(gout)[k]
    v = geo.tap_values(feats[l0], l0, 0)[k]
    wl = float(wu.reshape(geo.K, -1)[k, l0])
    H, W = hws[l0]
    S, N, _, _, C = feats[0].shape
    wrong = {}
    gf = [r.clone() for r in ref["feat"][0]]
    img = int(geo.img[k])
    gf[l0].view(S * N, H, W, C)[img, hi[k], wi[k]] -= float(tw[k]) * wl * g
    wrong["feat"] = gf
    dot = float((g * v).sum())
    gl = ref["loc"][0].clone().reshape(-1, 3)
    gl[k, 0] -= (W - 1) * wl * float(dw[k]) * dot
    gl[k, 1] -= (H - 1) * wl * float(dh[k]) * dot
    wrong["loc"] = gl.reshape(ref["loc"][0].shape)
    if "w" in ref:
        gw = ref["w"][0].clone().reshape(geo.K, -1)
        gw[k, l0] -= float(tw[k]) * dot
        wrong["w"] = gw.reshape(ref["w"][0].shape)
    return wrong


def msmv_compare(name, ref, got_feats, got_loc, got_w, feats, gout, got_out=None):
    """got_out: the forward's output, checked too (a non-finite location contributes what FAR does: nothing)"""
    hws = [tuple(f.shape[2:4]) for f in feats]
    if got_out is not None:
        check(f"{name} out", "feat", got_out, *ref["out"])
    for l in range(len(feats)):
        check(f"{name} feat{l}", "feat", got_feats[l], ref["feat"][0][l], ref["feat"][1][l])
    check(f"{name} loc", "loc", got_loc, *ref["loc"])
    assert bool((got_loc[..., 2] == 0).all())
    if got_w is not None:
        check(f"{name} w", "w", got_w, *ref["w"])
    wrong = msmv_drop_one_tap(ref, feats, gout, hws)
    must_fail(f"{name} feat", "feat", torch.cat([g.flatten() for g in got_feats]),
              torch.cat([g.flatten() for g in wrong["feat"]]), torch.cat([a.flatten() for a in ref["feat"][1]]))
    must_fail(f"{name} loc", "loc", got_loc, wrong["loc"], ref["loc"][1])
    if got_w is not None:
        must_fail(f"{name} w", "w", got_w, wrong["w"], ref["w"][1])


HWS = {1: [(9, 17)], 2: [(9, 17), (1, 9)], 3: [(9, 17), (5, 9), (9, 1)], 4: [(9, 17), (5, 9), (1, 9), (9, 1)],
       5: [(9, 17), (5, 9), (3, 5), (1, 9), (9, 1)],
       8: [(9, 17), (5, 9), (3, 5), (1, 9), (9, 1), (2, 3), (17, 5), (5, 2)]}


def _msmv_edge_points(N):
    """(u, v, z) rows; level 0 is 9 x 17 (H-1 = 8, W-1 = 16): every listed coordinate is exact in float32"""
    e = []
    b = float(np.nextafter(np.float32(9 / 8), np.float32(0)))          # h = 9 - eps: inside
    bw = float(np.nextafter(np.float32(17 / 16), np.float32(0)))
    for u, v in ((5 / 16, 3 / 8), (0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.3, -0.5 / 8), (-0.5 / 16, 0.7), (0.4, -1 / 8),
                 (-1 / 16, 0.4), (0.6, 9 / 8), (17 / 16, 0.6), (0.55, b), (bw, 0.45), (b, b),
                 (math.nan, 0.5), (0.5, math.nan), (math.inf, 0.5), (0.5, -math.inf), (-math.inf, math.inf)):
        e.append((u, v, 0.0))
    if N > 1:
        z_half = [z for z in (0.5, 0.1, 0.3, 0.7, 0.9) if np.float32(z) * np.float32(N - 1) % 1 == 0.5]
        assert z_half, N
        for z in z_half:
            e.append((0.37, 0.61, z))
    return e


def msmv_case(seed, S, N, Q, P, C, hws, edges=True):
    rng = np.random.default_rng(seed)
    feats = [torch.from_numpy(rng.standard_normal((S, N, h, w, C), dtype=np.float32)) for h, w in hws]
    loc = rng.random((S, Q, P, 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    loc[..., 2] = rng.integers(0, N, size=(S, Q, P)).astype(np.float32) / np.float32(max(N - 1, 1))
    if edges:
        e = np.array(_msmv_edge_points(N), dtype=np.float32)
        flat = loc.reshape(-1, 3)
        assert flat.shape[0] >= e.shape[0]
        flat[:e.shape[0]] = e
    w = torch.from_numpy(rng.random((S, Q, P, len(hws)), dtype=np.float32) + np.float32(0.05))
    gout = torch.from_numpy(rng.standard_normal((S, Q, C, P), dtype=np.float32))
    return feats, torch.from_numpy(loc), w, gout


def run_msmv(feats, loc, w, gout):
    from racformer_amd.msmv import msmv_sampling
    gf = [f.to(DEV).requires_grad_() for f in feats]
    gl, gw = loc.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    out = msmv_sampling(gf, gl, gw)
    out.backward(gout.to(DEV))
    return [f.grad for f in gf], gl.grad, gw.grad, out.detach()


@pytest.mark.parametrize("L", [2, 4, 5])
def test_msmv_bwd_c64_fast_path(L):
    feats, loc, w, gout = msmv_case(100 + L, S=2, N=6, Q=12, P=9, C=64, hws=HWS[L])
    ref = msmv_reference(feats, loc, w, gout, 6)
    gf, gl, gw, out = run_msmv(feats, loc, w, gout)
    msmv_compare(f"msmv c64 L{L}", ref, gf, gl, gw, feats, gout, out)


@pytest.mark.parametrize("N", [1, 6])
@pytest.mark.parametrize("L", [1, 3, 8])
@pytest.mark.parametrize("C", [1, 3, 8, 32, 128, 256])
def test_msmv_bwd_generic(C, L, N):
    feats, loc, w, gout = msmv_case(1000 + 10 * C + L + N, S=2, N=N, Q=5, P=5, C=C, hws=HWS[L])
    ref = msmv_reference(feats, loc, w, gout, N)
    gf, gl, gw, out = run_msmv(feats, loc, w, gout)
    msmv_compare(f"msmv generic C{C}", ref, gf, gl, gw, feats, gout, out)


def test_msmv_bwd_generic_past_the_grid():
    """1,152,000 points: more than the 4096 x 256 threads of the launch, so the grid-stride loop runs a second pass"""
    S, Q, P = 32, 900, 40
    assert S * Q * P > 4096 * 256
    feats, loc, w, gout = msmv_case(7, S=S, N=2, Q=Q, P=P, C=8, hws=[(9, 17)])
    ref = msmv_reference(feats, loc, w, gout, 2)
    gf, gl, gw, out = run_msmv(feats, loc, w, gout)
    msmv_compare("msmv generic 1.15M", ref, gf, gl, gw, feats, gout, out)


def test_msmv_bwd_collision():
    """every point of every query on one pixel neighbourhood: 100,000 atomic terms per tap pixel"""
    S, N, Q, P = 1, 1, 1000, 100
    feats, loc, w, gout = msmv_case(8, S=S, N=N, Q=Q, P=P, C=64, hws=HWS[2], edges=False)
    loc[..., 0], loc[..., 1] = 0.3, 0.6
    ref = msmv_reference(feats, loc, w, gout, N)
    gf, gl, gw, out = run_msmv(feats, loc, w, gout)
    msmv_compare("msmv c64 collision", ref, gf, gl, gw, feats, gout, out)


def test_msmv_bwd_autograd_plumbing():
    """expanded and permuted grad_output, a subset of inputs requiring grad, accumulation into .grad, and bit-identical
    single-writer gradients between runs"""
    from racformer_amd.msmv import msmv_sampling
    S, N, Q, P, C = 2, 6, 7, 9, 64
    feats, loc, w, _ = msmv_case(9, S=S, N=N, Q=Q, P=P, C=C, hws=HWS[4])
    # out.sum().backward(): grad_output is an expanded (stride 0) tensor of ones
    ones = torch.ones(S, Q, C, P)
    ref = msmv_reference(feats, loc, w, ones, N)
    gf = [f.to(DEV).requires_grad_() for f in feats]
    gl, gw = loc.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    msmv_sampling(gf, gl, gw).sum().backward()
    msmv_compare("msmv expanded gout", ref, [f.grad for f in gf], gl.grad, gw.grad, feats, ones)
    first = (gl.grad.clone(), gw.grad.clone())
    # a second backward accumulates: single-writer gradients are bit-identical run to run, so exactly twice the first
    msmv_sampling(gf, gl, gw).sum().backward()
    assert torch.equal(gl.grad, 2 * first[0]) and torch.equal(gw.grad, 2 * first[1])
    for l in range(len(feats)):
        check(f"msmv 2x feat{l}", "feat", gf[l].grad, 2 * ref["feat"][0][l], 2 * ref["feat"][1][l])
    # permuted grad_output: the loss reads the output through a permute
    rng = np.random.default_rng(10)
    G = torch.from_numpy(rng.standard_normal((S, Q, P, C), dtype=np.float32))
    ref = msmv_reference(feats, loc, w, G.permute(0, 1, 3, 2).contiguous(), N)
    gf = [f.to(DEV).requires_grad_() for f in feats]
    gl, gw = loc.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    out = msmv_sampling(gf, gl, gw)
    (out.permute(0, 1, 3, 2) * G.to(DEV)).sum().backward()
    msmv_compare("msmv permuted gout", ref, [f.grad for f in gf], gl.grad, gw.grad, feats, G.permute(0, 1, 3, 2))
    # only the locations require grad
    gl2 = loc.to(DEV).requires_grad_()
    out = msmv_sampling([f.to(DEV) for f in feats], gl2, w.to(DEV))
    (out.permute(0, 1, 3, 2) * G.to(DEV)).sum().backward()
    assert torch.equal(gl2.grad, gl.grad)


# ---------------------------------------------------------------------------------------------------------------- v2
def run_v2(feats, loc, w, gout, channels_first=False):
    from racformer_amd.msmv import msmv_sampling_v2
    fs = [f.permute(0, 4, 1, 2, 3).contiguous() if channels_first else f for f in feats]
    gf = [f.to(DEV).requires_grad_() for f in fs]
    gl, gw = loc.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    out = msmv_sampling_v2(gf, gl, gw, channels_first=channels_first)
    out.backward(gout.to(DEV))
    assert gw.grad is None
    grads = [f.grad.permute(0, 2, 3, 4, 1) if channels_first else f.grad for f in gf]
    return grads, gl.grad, out.detach()


@pytest.mark.parametrize("L,channels_first", [(2, False), (5, False), (4, True)])
def test_msmv_v2_bwd(L, channels_first):
    feats, loc, w, gout = msmv_case(200 + L, S=2, N=6, Q=12, P=9, C=64, hws=HWS[L])
    ref = msmv_reference(feats, loc, w, gout, 6, v2=True)
    gf, gl, out = run_v2(feats, loc, w, gout, channels_first)
    msmv_compare(f"v2 c64 L{L}{' cf' if channels_first else ''}", ref, gf, gl, None, feats, gout, out)


def test_msmv_v2_bwd_generic_past_the_grid():
    S, Q, P = 32, 900, 40
    feats, loc, w, gout = msmv_case(11, S=S, N=2, Q=Q, P=P, C=8, hws=HWS[2])
    ref = msmv_reference(feats, loc, w, gout, 2, v2=True)
    gf, gl, out = run_v2(feats, loc, w, gout)
    msmv_compare("v2 generic 1.15M", ref, gf, gl, None, feats, gout, out)


def test_msmv_v2_bwd_deterministic_loc():
    feats, loc, w, gout = msmv_case(12, S=2, N=6, Q=12, P=9, C=64, hws=HWS[4])
    _, a, _ = run_v2(feats, loc, w, gout)
    _, b, _ = run_v2(feats, loc, w, gout)
    assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------------------- msda
def _msda_layout(shapes, gap, tail):
    starts, k = [], gap
    for h, w in shapes:
        starts.append(k)
        k += h * w + 2                    # two unused keys after every level
    return starts, k + tail


def _msda_edge_points():
    """(x, y) rows; level 0 is 8 x 16 (align_corners=False: h = y*8 - 0.5, w = x*16 - 0.5), exact in float32"""
    hb = float(np.nextafter(np.float32(8.5 / 8), np.float32(0)))       # h = 8 - eps: inside
    wb = float(np.nextafter(np.float32(16.5 / 16), np.float32(0)))
    return [(3.5 / 16, 2.5 / 8), (0.0, 0.0), (1.0, 1.0), (0.5 / 16, 0.25 / 8), (0.3, 0.25 / 8), (-0.5 / 16, 0.4),
            (0.4, -0.5 / 8), (16.5 / 16, 0.6), (0.6, 8.5 / 8), (wb, 0.3), (0.45, hb), (wb, hb),
            (math.nan, 0.5), (0.5, math.nan), (math.inf, 0.5), (0.5, -math.inf)]


def msda_case(seed, bs, Q, heads, dim, P, shapes, edges=True):
    rng = np.random.default_rng(seed)
    starts, keys = _msda_layout(shapes, gap=3, tail=5)
    L = len(shapes)
    value = torch.from_numpy(rng.standard_normal((bs, keys, heads, dim), dtype=np.float32))
    loc = rng.random((bs, Q, heads, L, P, 2), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    if edges:
        e = np.array(_msda_edge_points(), dtype=np.float32)
        lv0 = loc[:, :, :, 0].reshape(-1, 2)         # level 0 of the first points
        assert lv0.shape[0] >= e.shape[0]
        lv0[:e.shape[0]] = e
        loc[:, :, :, 0] = lv0.reshape(loc[:, :, :, 0].shape)
    attn = torch.from_numpy(rng.random((bs, Q, heads, L, P), dtype=np.float32) + np.float32(0.05))
    gout = torch.from_numpy(rng.standard_normal((bs, Q, heads * dim), dtype=np.float32))
    return value, [list(s) for s in shapes], starts, torch.from_numpy(loc), attn, gout


def msda_reference(value, shapes, starts, loc, attn, gout):
    bs, keys, heads, dim = value.shape
    _, Q, _, L, P, _ = loc.shape
    loc_o = _finite_for_oracle(loc).double()
    g64 = gout.double()
    v64, l64, a64 = value.double().requires_grad_(), loc_o.clone().requires_grad_(), attn.double().requires_grad_()
    fwd = R.msda_torch(v64, shapes, starts, l64, a64, f32_coords=True)
    fwd.backward(g64)
    va, aa = value.double().abs().requires_grad_(), attn.double().abs().requires_grad_()
    fwd_a = R.msda_torch(va, shapes, starts, loc_o, aa, f32_coords=True)
    fwd_a.backward(g64.abs())
    # loc magnitude and the geometry of the negative control
    ga = g64.abs().reshape(bs, Q, heads, dim)
    A_loc = torch.zeros(bs, Q, heads, L, P, 2, dtype=torch.float64)
    geo = {}
    for l, (H, W) in enumerate(shapes):
        x, y = loc[:, :, :, l, :, 0].reshape(-1), loc[:, :, :, l, :, 1].reshape(-1)
        _, taps = _taps(_f32c(y, H, 0.5), _f32c(x, W, 0.5), H, W)
        bi = torch.arange(bs).repeat_interleave(Q * heads * P)
        hi_ = torch.arange(heads).repeat_interleave(P).repeat(bs * Q)
        qi = torch.arange(Q).repeat_interleave(heads * P).repeat(bs)
        T = torch.zeros(x.shape[0], dtype=torch.float64)
        for hi, wi, tw, dh, dw, ok in taps:
            v = value.double()[bi, starts[l] + hi * W + wi, hi_]
            T += torch.where(ok, (v.abs() * ga[bi, qi, hi_]).sum(-1), torch.zeros_like(T))
        a = attn.double().abs()[:, :, :, l].reshape(-1)
        A_loc[:, :, :, l, :, 0] = (W * a * T).reshape(bs, Q, heads, P)
        A_loc[:, :, :, l, :, 1] = (H * a * T).reshape(bs, Q, heads, P)
        geo[l] = (taps, bi, qi, hi_)
    return {"feat": (v64.grad, va.grad), "w": (a64.grad, aa.grad), "loc": (l64.grad, A_loc), "geo": geo,
            "out": (fwd.detach(), fwd_a.detach())}


def msda_drop_one_tap(ref, value, shapes, starts, loc, attn, gout):
    bs, keys, heads, dim = value.shape
    _, Q, _, L, P, _ = loc.shape
    taps, bi, qi, hd = ref["geo"][0]
    hi, wi, tw, dh, dw, ok = taps[0]
    cand = ok.nonzero().flatten()[:64]
    assert cand.numel() > 0
    k = int(cand[torch.argmax(tw[cand])])
    b, q, h = int(bi[k]), int(qi[k]), int(hd[k])
    p = k % P
    H, W = shapes[0]
    g = gout.double().reshape(bs, Q, heads, dim)[b, q, h]
    key = starts[0] + int(hi[k]) * W + int(wi[k])
    v = value.double()[b, key, h]
    at = float(attn[b, q, h, 0, p])
    dot = float((g * v).sum())
    wrong = {"feat": ref["feat"][0].clone(), "w": ref["w"][0].clone(), "loc": ref["loc"][0].clone()}
    wrong["feat"][b, key, h] -= float(tw[k]) * at * g
    wrong["w"][b, q, h, 0, p] -= float(tw[k]) * dot
    wrong["loc"][b, q, h, 0, p, 0] -= W * at * float(dw[k]) * dot
    wrong["loc"][b, q, h, 0, p, 1] -= H * at * float(dh[k]) * dot
    return wrong


def run_msda(value, shapes, starts, loc, attn, gout, need=(True, True, True)):
    from racformer_amd.msda import MultiScaleDeformableAttnFunction_fp32 as F32
    v, l, a = value.to(DEV).requires_grad_(need[0]), loc.to(DEV).requires_grad_(need[1]), attn.to(DEV).requires_grad_(need[2])
    out = F32.apply(v, torch.tensor(shapes, device=DEV), torch.tensor(starts, device=DEV), l, a, 64)
    out.backward(gout.to(DEV))
    return v.grad, l.grad, a.grad, out.detach()


def msda_compare(name, ref, got, case):
    """got: (grad_value, grad_loc, grad_attn[, forward output])"""
    gv, gl, ga, *fwd = got
    if fwd:
        check(f"{name} out", "feat", fwd[0], *ref["out"])
    check(f"{name} value", "feat", gv, *ref["feat"])
    check(f"{name} loc", "loc", gl, *ref["loc"])
    check(f"{name} attn", "w", ga, *ref["w"])
    wrong = msda_drop_one_tap(ref, *case)
    must_fail(f"{name} value", "feat", gv, wrong["feat"], ref["feat"][1])
    must_fail(f"{name} loc", "loc", gl, wrong["loc"], ref["loc"][1])
    must_fail(f"{name} attn", "w", ga, wrong["w"], ref["w"][1])


MSDA_SHAPES = {1: [(8, 16)], 4: [(8, 16), (4, 8), (1, 8), (8, 1)]}


@pytest.mark.parametrize("L", [1, 4])
@pytest.mark.parametrize("heads", [1, 4, 8])
def test_msda_bwd_d64(heads, L):
    case = msda_case(300 + heads + L, bs=2, Q=5, heads=heads, dim=64, P=4, shapes=MSDA_SHAPES[L])
    ref = msda_reference(*case)
    msda_compare(f"msda d64 h{heads} L{L}", ref, run_msda(*case), case)


@pytest.mark.parametrize("dim", [3, 8, 32, 128])
def test_msda_bwd_generic(dim):
    case = msda_case(400 + dim, bs=2, Q=5, heads=2, dim=dim, P=4, shapes=MSDA_SHAPES[4])
    ref = msda_reference(*case)
    msda_compare(f"msda generic d{dim}", ref, run_msda(*case), case)


def test_msda_bwd_generic_past_the_grid():
    """1,152,000 samples: more than the 4096 x 256 threads of the launch"""
    bs, Q, heads, L, P = 1, 4500, 2, 2, 64
    assert bs * Q * heads * L * P > 4096 * 256
    case = msda_case(13, bs=bs, Q=Q, heads=heads, dim=3, P=P, shapes=[(8, 16), (4, 8)])
    ref = msda_reference(*case)
    msda_compare("msda generic 1.15M", ref, run_msda(*case), case)


def test_msda_bwd_collision():
    """100,000 samples on one location: every tap pixel takes 100,000 atomic terms"""
    case = list(msda_case(14, bs=1, Q=2000, heads=1, dim=64, P=50, shapes=[(8, 16)], edges=False))
    case[3][..., 0], case[3][..., 1] = 0.37, 0.61
    ref = msda_reference(*case)
    msda_compare("msda d64 collision", ref, run_msda(*case), case)


def test_msda_bwd_autograd_plumbing():
    from racformer_amd.msda import MultiScaleDeformableAttnFunction_fp32 as F32
    value, shapes, starts, loc, attn, _ = case = msda_case(15, bs=2, Q=5, heads=4, dim=64, P=4, shapes=MSDA_SHAPES[4])
    ones = torch.ones(2, 5, 4 * 64)
    ref = msda_reference(value, shapes, starts, loc, attn, ones)
    v, l, a = value.to(DEV).requires_grad_(), loc.to(DEV).requires_grad_(), attn.to(DEV).requires_grad_()
    sh, st = torch.tensor(shapes, device=DEV), torch.tensor(starts, device=DEV)
    F32.apply(v, sh, st, l, a, 64).sum().backward()                      # expanded grad_output
    msda_compare("msda expanded gout", ref, (v.grad, l.grad, a.grad), (value, shapes, starts, loc, attn, ones))
    first = (l.grad.clone(), a.grad.clone())
    F32.apply(v, sh, st, l, a, 64).sum().backward()                      # accumulates
    assert torch.equal(l.grad, 2 * first[0]) and torch.equal(a.grad, 2 * first[1])
    check("msda 2x value", "feat", v.grad, 2 * ref["feat"][0], 2 * ref["feat"][1])
    # permuted grad_output, and only the attention weights requiring grad
    G = torch.from_numpy(np.random.default_rng(16).standard_normal((5, 2, 4 * 64), dtype=np.float32))
    ref = msda_reference(value, shapes, starts, loc, attn, G.permute(1, 0, 2).contiguous())
    a2 = attn.to(DEV).requires_grad_()
    out = F32.apply(value.to(DEV), sh, st, loc.to(DEV), a2, 64)
    (out.permute(1, 0, 2) * G.to(DEV)).sum().backward()
    check("msda permuted attn", "w", a2.grad, *ref["w"])
    _, _, ga, _ = run_msda(value, shapes, starts, loc, attn, G.permute(1, 0, 2).contiguous())
    assert torch.equal(ga, a2.grad)


# ------------------------------------------------------------------------------------------------------------ bev_pool
def bev_case(seed, c, D=100, H=2, W=3, grid=2):
    """LSS-shaped: B = N = 1, 90 % of D*H*W points kept; every feature cell is read by ~90 points (backward intervals
    longer than 64 lanes) and every BEV cell of the 2 x 2 grid pools ~135 (forward intervals as long)"""
    rng = np.random.default_rng(seed)
    depth = torch.from_numpy(rng.random((1, 1, D, H, W), dtype=np.float32))
    feat = torch.from_numpy(rng.standard_normal((1, 1, H, W, c), dtype=np.float32))
    keep = rng.random(D * H * W) < 0.9
    rd = np.nonzero(keep)[0].astype(np.int32)
    rf = (rd % (H * W)).astype(np.int32)
    rb = rng.integers(0, grid * grid, size=rd.shape[0]).astype(np.int32)
    order = np.argsort(rb, kind="stable")
    rd, rf, rb = (torch.from_numpy(a[order].astype(np.int32)) for a in (rd, rf, rb))
    _, counts = torch.unique_consecutive(rb, return_counts=True)
    starts, lengths = (torch.cumsum(counts, 0) - counts).int(), counts.int()
    shape = (1, 1, grid, grid, c)
    gout = torch.from_numpy(rng.standard_normal((1, c, 1, grid, grid), dtype=np.float32))
    return depth, feat, rd, rf, rb, shape, starts, lengths, gout


def run_bev(depth, feat, rd, rf, rb, shape, starts, lengths, gout):
    from racformer_amd.bev_pool import bev_pool_v2
    d, f = depth.to(DEV).requires_grad_(), feat.to(DEV).requires_grad_()
    bev_pool_v2(d, f, rd.to(DEV), rf.to(DEV), rb.to(DEV), shape, starts.to(DEV), lengths.to(DEV)).backward(gout.to(DEV))
    return d.grad, f.grad


@pytest.mark.parametrize("c", [256, 320, 128, 160, 64, 80, 6])
def test_bev_pool_bwd(c):
    """c = 256 / 320: 64 lanes whole / partial; 128 / 160: 32 lanes; 64 / 80: 16 lanes; 6: the scalar kernel"""
    depth, feat, rd, rf, rb, shape, starts, lengths, gout = case = bev_case(500 + c, c)
    assert int(torch.bincount(rf.long()).max()) > 64 and int(lengths.max()) > 64
    d64, f64 = depth.double().requires_grad_(), feat.double().requires_grad_()
    R.bev_pool_v2(d64, f64, rd, rf, rb, shape, starts, lengths).backward(gout.double())
    # magnitudes: depth gradients from |feat| and |grad_out|, feature gradients from |depth| and |grad_out|
    da, fa = depth.double().abs().requires_grad_(), feat.double().abs().requires_grad_()
    R.bev_pool_v2(da, fa, rd, rf, rb, shape, starts, lengths).backward(gout.double().abs())
    Ad, Af = da.grad, fa.grad
    gd, gf = run_bev(*case)
    check(f"bev c{c} depth", "w", gd, d64.grad, Ad)
    check(f"bev c{c} feat", "feat", gf, f64.grad, Af)
    # single writer per element: bit-identical between runs
    gd2, gf2 = run_bev(*case)
    assert torch.equal(gd, gd2) and torch.equal(gf, gf2)
    # negative control: one point of the first interval dropped
    i = int(starts[0])
    og = gout.double().permute(0, 2, 3, 4, 1).reshape(-1, c)[int(rb[i])]
    wd, wf = d64.grad.clone(), f64.grad.clone()
    wd.view(-1)[int(rd[i])] = 0.0
    wf.view(-1, c)[int(rf[i])] -= float(depth.view(-1)[int(rd[i])]) * og
    must_fail(f"bev c{c} depth", "w", gd, wd, Ad)
    must_fail(f"bev c{c} feat", "feat", gf, wf, Af)
