"""Autograd through sampling_4d (both modes) and BEVSelfAttention on the MI355X, with the backward kernels reading the gradient
in sampling_4d's own [B,Q,G,T*P,C] layout (rac_msmv_bwd_ex / rac_msmv_v2_bwd_ex).

  * the reference's own autograd (tests/golden/sampling4d_grad_small.npz) in both modes, C = 8 and C = 64;
  * element-wise against float64 with the error model of tests/test_backward_f64_gpu.py (err <= K * 2^-24 * A, the same K,
    its helpers): feature and weight gradients, and the location gradient captured at the autograd Function's boundary,
    for C = 64 and C = 8, L = 2 / 4 / 5, edge locations, a launch past the generic kernels' 4096-block grid, imposed views
    and NaN / inf sample points, each with its negative control;
  * the two gradient layouts against each other, and the entry points without _ex against a pin of the parent build
    (tests/golden/msmv_bwd_pin.npz): single-writer gradients bit for bit;
  * BEVSelfAttention against the float64 oracle composition, every parameter and input;
  * bit-identical repeat runs."""
import os

import numpy as np
import pytest
import torch

from oracle import restate as R
from racformer_amd import _lib, synthetic as syn
from racformer_amd import transformer as T
from racformer_amd.msmv import msmv_backward, msmv_v2_backward
from test_backward_f64_gpu import HWS, check, msmv_case, msmv_compare, msmv_reference
from test_sampling4d_grad_cpu import SCALE, TOL, _bev_case, to_bqgtpc, to_sqcp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return torch.from_numpy(np.asarray(a)).clone()


# --------------------------------------------------------------------------------------------- 4. reference golden
# tests/test_backward.py's operator-level tolerances: the golden's generic case (C = 8) 2e-5 / 2e-4, its C = 64 fast path
# against the oracle 5e-5 / 5e-4; sample_points take the location tolerance times SCALE (projection chain, see
# tests/test_sampling4d_grad_cpu.py, where |d(u|v)/d point| <= 0.5 on these fixtures is derived).
GOLDEN_TOL = {"l4_": TOL, "l5_": {"feat": 5e-5, "w": 5e-5, "loc": 5e-4}}


@pytest.mark.parametrize("pre", ["l4_", "l5_"])
@pytest.mark.parametrize("aggregate", [True, False])
def test_sampling_4d_gradients_match_the_reference(golden_dir, pre, aggregate):
    g = np.load(os.path.join(golden_dir, "sampling4d_grad_small.npz"))
    mode = "agg_" if aggregate else "hard_"
    tol = GOLDEN_TOL[pre]
    H, W = (int(x) for x in g[pre + "image_hw"])
    L = sum(1 for k in g.files if k.startswith(pre + "feat"))
    feats = [t(g[f"{pre}feat{i}"]).to(DEV).requires_grad_() for i in range(L)]
    pts = t(g[pre + "pts"]).to(DEV).requires_grad_()
    sw = t(g[pre + "scale_weights"]).to(DEV).requires_grad_()
    res = T.sampling_4d(pts, feats, sw, t(g[pre + "lidar2img"]).to(DEV), H, W, aggregate=aggregate)
    final = res if aggregate else res[0]
    assert final.grad_fn is not None
    (final * t(g[pre + "gout"]).to(DEV)).sum().backward()
    for i, f in enumerate(feats):
        assert (f.grad.cpu() - t(g[f"{pre}{mode}gfeat{i}"])).abs().max().item() < tol["feat"], i
    if aggregate:
        assert (sw.grad.cpu() - t(g[pre + mode + "gsw"])).abs().max().item() < tol["w"]
    else:
        assert sw.grad is None
    assert (pts.grad.cpu() - t(g[pre + mode + "gpts"])).abs().max().item() < tol["loc"] * SCALE


def test_bf16_features_refuse_the_backward():
    """the backward kernels are float32 only: bf16 features with a gradient requested raise, they are not cut off"""
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "sampling4d_grad_small.npz"))
    H, W = (int(x) for x in g["l5_image_hw"])
    feats = [t(g[f"l5_feat{i}"]).to(DEV).to(torch.bfloat16).requires_grad_() for i in range(5)]
    pts = t(g["l5_pts"]).to(DEV).requires_grad_()
    for aggregate in (True, False):
        res = T.sampling_4d(pts, feats, t(g["l5_scale_weights"]).to(DEV), t(g["l5_lidar2img"]).to(DEV), H, W,
                            aggregate=aggregate)
        final = res if aggregate else res[0]
        with pytest.raises(RuntimeError, match="float32 features only"):
            final.sum().backward()


# --------------------------------------------------------------------------------------------- 5. float64, element-wise
def s4d_case(seed, B, Q, Tn, G, P, N, C, hws, nonfinite=False):
    """seeded sampling_4d inputs on a ring rig: points 3-25 m around it (most seen by a camera), the first query's first
    points high above it (seen by none); nonfinite: NaN / +-inf coordinates in some points"""
    rng = np.random.default_rng(seed)
    H, W = 64, 176
    S = B * Tn * G
    feats = [torch.from_numpy(rng.standard_normal((S, N, h, w, C), dtype=np.float32)) for h, w in hws]
    ang = rng.random((B, Q, Tn, G, P)) * 2 * np.pi
    r = 3.0 + rng.random((B, Q, Tn, G, P)) * 22.0
    z = rng.standard_normal((B, Q, Tn, G, P)) * 0.5 + 0.5
    pts = np.stack([r * np.cos(ang), r * np.sin(ang), z], -1).astype(np.float32)
    pts[0, 0, :, :, :2, 2] = 500.0
    if nonfinite:
        bad = [(np.nan, 1.0, 0.5), (np.inf, 2.0, 0.5), (3.0, -np.inf, 0.5), (4.0, 1.0, np.nan), (np.nan, np.nan, np.nan)]
        pts[0, -1, 0, 0, :len(bad)] = np.array(bad, dtype=np.float32)
    sw = rng.standard_normal((B, Q, G, Tn, P, len(hws)), dtype=np.float32)
    sw = (np.exp(sw) / np.exp(sw).sum(-1, keepdims=True)).astype(np.float32)
    l2i = np.asarray(syn.ring_lidar2img(Tn, N, (H, W)), np.float32)[None].repeat(B, 0)
    gout = rng.standard_normal((B, Q, G, Tn * P, C), dtype=np.float32)
    return dict(feats=feats, pts=torch.from_numpy(pts), sw=torch.from_numpy(sw), l2i=torch.from_numpy(l2i), hw=(H, W),
                gout=torch.from_numpy(gout), N=N, Tn=Tn, G=G)


def run_s4d(case, aggregate, monkeypatch, view_in=None):
    """sampling_4d forward + backward on the GPU; -> (feature grads, [(loc, w) handed to the autograd Function])"""
    seen = []
    orig = T._Sampling4DGather.apply

    def spy(agg, Tn, G, loc, w, *feats):
        loc.retain_grad()
        if w.requires_grad:
            w.retain_grad()
        seen.append((loc, w))
        return orig(agg, Tn, G, loc, w, *feats)

    monkeypatch.setattr(T._Sampling4DGather, "apply", spy)
    gf = [f.to(DEV).requires_grad_() for f in case["feats"]]
    pts, sw = case["pts"].to(DEV).requires_grad_(), case["sw"].to(DEV).requires_grad_()
    H, W = case["hw"]
    res = T.sampling_4d(pts, gf, sw, case["l2i"].to(DEV), H, W, aggregate=aggregate,
                        view_in=None if view_in is None else view_in.to(DEV))
    final = res if aggregate else res[0]
    final.backward(case["gout"].to(DEV))
    monkeypatch.undo()
    assert len(seen) == 1
    return [f.grad for f in gf], seen[0]


def compare_s4d(name, case, aggregate, monkeypatch, view_in=None):
    gf, (loc, w) = run_s4d(case, aggregate, monkeypatch, view_in)
    gout = to_sqcp(case["gout"], case["Tn"], case["G"])
    ref = msmv_reference(case["feats"], loc.detach().cpu(), w.detach().cpu(), gout, case["N"], v2=not aggregate)
    msmv_compare(name, ref, gf, loc.grad, w.grad if aggregate else None, case["feats"], gout)
    return loc, w


@pytest.mark.parametrize("aggregate", [True, False])
@pytest.mark.parametrize("L", [2, 4, 5])
@pytest.mark.parametrize("C", [64, 8])
def test_sampling_4d_float64(C, L, aggregate, monkeypatch):
    case = s4d_case(200 + C + L, B=2, Q=30, Tn=2, G=3, P=8, N=6, C=C, hws=HWS[L])
    compare_s4d(f"s4d {'agg' if aggregate else 'hard'} C{C} L{L}", case, aggregate, monkeypatch)


@pytest.mark.parametrize("aggregate", [True, False])
def test_sampling_4d_float64_imposed_views(aggregate, monkeypatch):
    case = s4d_case(300, B=2, Q=30, Tn=2, G=2, P=8, N=6, C=64, hws=HWS[4])
    forced = torch.from_numpy(np.random.default_rng(5).integers(0, 6, size=(8, 30, 8)).astype(np.uint8))
    loc, _ = compare_s4d(f"s4d {'agg' if aggregate else 'hard'} view_in", case, aggregate, monkeypatch, view_in=forced)
    assert torch.equal(R._round_half_away(loc.detach().cpu()[..., 2] * 5).to(torch.uint8), forced)


@pytest.mark.parametrize("aggregate", [True, False])
@pytest.mark.parametrize("C", [64, 8])
def test_sampling_4d_float64_nonfinite_points(C, aggregate, monkeypatch):
    """NaN / +-inf sample points: zero location gradients at the gather, and no NaN in any feature or weight gradient"""
    case = s4d_case(400 + C, B=1, Q=20, Tn=2, G=2, P=8, N=6, C=C, hws=HWS[4], nonfinite=True)
    loc, w = compare_s4d(f"s4d {'agg' if aggregate else 'hard'} nonfinite C{C}", case, aggregate, monkeypatch)
    bad = ~torch.isfinite(loc.detach()[..., :2]).all(-1)
    assert int(bad.sum()) >= 5
    assert bool((loc.grad[bad] == 0).all())
    if aggregate:
        assert bool(torch.isfinite(w.grad).all()) and bool((w.grad[bad] == 0).all())


def run_gather(feats, loc, w, gout_bq, Tn, G, aggregate):
    """the autograd Function of sampling_4d on its own: -> feature, location and weight gradients"""
    gf = [f.to(DEV).requires_grad_() for f in feats]
    gl, gw = loc.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    T._Sampling4DGather.apply(aggregate, Tn, G, gl, gw, *gf).backward(gout_bq.to(DEV))
    return [f.grad for f in gf], gl.grad, gw.grad


@pytest.mark.parametrize("aggregate", [True, False])
@pytest.mark.parametrize("C,L", [(64, 2), (64, 4), (64, 5), (8, 3), (32, 8)])
def test_gather_float64_edge_locations(C, L, aggregate):
    """the Function alone on the edge locations of test_backward_f64_gpu.py (exact taps, -1 / H bounds, NaN / inf, halfway
    cameras), B = 2, T = 2, G = 3"""
    Tn, G = 2, 3
    feats, loc, w, gout = msmv_case(500 + C + L, S=2 * Tn * G, N=6, Q=5, P=7, C=C, hws=HWS[L])
    gf, gl, gw = run_gather(feats, loc, w, to_bqgtpc(gout, Tn, G).contiguous(), Tn, G, aggregate)
    ref = msmv_reference(feats, loc, w, gout, 6, v2=not aggregate)
    msmv_compare(f"gather {'agg' if aggregate else 'hard'} edges C{C} L{L}", ref, gf, gl, gw if aggregate else None, feats, gout)
    assert aggregate or gw is None


@pytest.mark.parametrize("aggregate", [True, False])
def test_gather_float64_past_the_grid(aggregate):
    """1,152,000 points: more than the 4096 x 256 threads of the generic kernels' launch"""
    Tn, G, Q, P = 8, 4, 900, 40
    feats, loc, w, gout = msmv_case(7, S=Tn * G, N=2, Q=Q, P=P, C=8, hws=[(9, 17), (5, 9)])
    assert Tn * G * Q * P > 4096 * 256
    gf, gl, gw = run_gather(feats, loc, w, to_bqgtpc(gout, Tn, G).contiguous(), Tn, G, aggregate)
    ref = msmv_reference(feats, loc, w, gout, 2, v2=not aggregate)
    msmv_compare(f"gather {'agg' if aggregate else 'hard'} 1.15M", ref, gf, gl, gw if aggregate else None, feats, gout)


# --------------------------------------------------------------------------------------------- 6. layouts agree
@pytest.mark.parametrize("v2,cf", [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("C,L", [(64, 2), (64, 4), (64, 5), (8, 4)])
def test_layouts_agree(C, L, v2, cf):
    """BQGTPC read directly against the permuted SQCP copy: grad_loc / grad_w bit-identical, features within the atomics bound"""
    Tn, G = 3, 2
    feats, loc, w, gout = msmv_case(600 + C + L, S=2 * Tn * G, N=6, Q=9, P=7, C=C, hws=HWS[L])
    ref = msmv_reference(feats, loc, w, gout, 6, v2=v2)
    df = [f.to(DEV) for f in feats]
    if cf:
        df = [f.permute(0, 4, 1, 2, 3).contiguous() for f in df]
    dl, dw = loc.to(DEV), w.to(DEV)
    bq = to_bqgtpc(gout, Tn, G).contiguous().to(DEV)
    sq = to_sqcp(bq, Tn, G).contiguous()
    assert torch.equal(sq.cpu(), gout)
    res = {}
    for name, g, kw in (("bq", bq, dict(grad_layout=_lib.OUT_BQGTPC, num_frames=Tn, num_groups=G)), ("sq", sq, {})):
        if v2:
            res[name] = (*msmv_v2_backward(g, df, dl, dw, channels_first=cf, **kw), None)
        else:
            res[name] = msmv_backward(g, df, dl, dw, **kw)
    (fb, lb, wb), (fs, ls, ws) = res["bq"], res["sq"]
    assert torch.equal(lb, ls)
    assert v2 or torch.equal(wb, ws)
    for l in range(L):
        a, b = fb[l], fs[l]
        if cf:
            a, b = a.permute(0, 2, 3, 4, 1), b.permute(0, 2, 3, 4, 1)
        check(f"layouts feat{l}", "feat", a, b.double(), ref["feat"][1][l])
        check(f"layouts ref feat{l}", "feat", a, ref["feat"][0][l], ref["feat"][1][l])


def test_entry_points_match_the_parent_build(golden_dir):
    """rac_msmv_bwd / rac_msmv_v2_bwd, and the _ex entry points in both layouts, return the pinned grad_loc / grad_w of the
    parent build bit for bit (tests/golden/gen_msmv_bwd_pin.py): every backward kernel instance"""
    from golden import gen_msmv_bwd_pin as pin
    d = dict(np.load(os.path.join(golden_dir, "msmv_bwd_pin.npz")))
    lib = _lib.lib()
    for name, C, L, v2, cf in pin.CASES:
        gloc, gw = pin.run_old(lib, d, name, C, L, v2, cf)                        # the old entry points, this build
        assert np.array_equal(gloc, d[name + "_gloc"], equal_nan=True), name
        assert v2 or np.array_equal(gw, d[name + "_gw"]), name
        feats = [t(d[f"c{C}_feat{l}"]).to(DEV) for l in range(L)]
        if cf:
            feats = [f.permute(0, 4, 1, 2, 3).contiguous() for f in feats]
        loc, w = t(d["loc"]).to(DEV), t(np.ascontiguousarray(d["w"][..., :L])).to(DEV)
        gout = t(d[f"c{C}_gout"])
        for g, kw in ((gout.to(DEV), {}),
                      (to_bqgtpc(gout, pin.T_, pin.G_).contiguous().to(DEV),
                       dict(grad_layout=_lib.OUT_BQGTPC, num_frames=pin.T_, num_groups=pin.G_))):
            if v2:
                _, gl = msmv_v2_backward(g, feats, loc, w, channels_first=cf, **kw)
            else:
                _, gl, gww = msmv_backward(g, feats, loc, w, **kw)
                assert np.array_equal(gww.cpu().numpy(), d[name + "_gw"]), (name, kw)
            assert np.array_equal(gl.cpu().numpy(), d[name + "_gloc"]), (name, kw)


# --------------------------------------------------------------------------------------------- 7. BEVSelfAttention
@pytest.mark.parametrize("C,heads", [(256, 4), (32, 4)])
def test_bev_self_attention_float64(C, heads, monkeypatch):
    """every parameter and input gradient against the float64 oracle composition (bev_self_attention with msda_torch, quirk Q2
    included): dim 64 takes rac_msda_bwd's d64 kernel, dim 8 the generic one.  Bound per gradient: 1e-4 of its largest float64
    magnitude -- the float32 chain (two GEMMs, the value scatter, the softmax) rounds a few dozen times per element"""
    mod, query, maps, loc, aw, hw = _bev_case(seed=11, B=2, Q=40, C=C, heads=heads, Tq=3, P=12, H=9, W=13)
    mod = mod.to(DEV)
    ins = [x.to(DEV).requires_grad_() for x in (query, maps, loc, aw)]
    out = mod(ins[0], ins[1], ins[2], ins[3], spatial_shapes=hw)
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(3))
    out.backward(gout.to(DEV))
    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in mod.state_dict().items()}
    ref_ins = [x.detach().double().requires_grad_() for x in (query, maps, loc, aw)]
    monkeypatch.setattr(R, "msda", lambda *a: R.msda_torch(*a))
    ref = R.bev_self_attention({"m." + k: v for k, v in sd.items()}, "m", *ref_ins, heads=heads)
    assert (out.detach().cpu().double() - ref.detach()).abs().max().item() < 1e-4 * ref.abs().max().item()
    ref.backward(gout.double())
    named = list(zip(("query", "value maps", "sampling_locations", "attention_weights"), ins, ref_ins))
    named += [(k, p, sd[k]) for k, p in mod.named_parameters()]
    for name, got, want in named:
        scale = want.grad.abs().max().item()
        err = (got.grad.cpu().double() - want.grad).abs().max().item()
        print(f"bev C{C} {name}: err {err:.3e} / max {scale:.3e} = {err / scale:.2e}")
        assert scale > 0 and err <= 1e-4 * scale, (name, err, scale)


# --------------------------------------------------------------------------------------------- 8. repeat runs
@pytest.mark.parametrize("aggregate", [True, False])
def test_repeat_runs_bit_identical(aggregate, monkeypatch):
    case = s4d_case(800, B=2, Q=60, Tn=2, G=2, P=12, N=6, C=64, hws=HWS[4])
    runs = []
    for _ in range(2):
        _, (loc, w) = run_s4d(case, aggregate, monkeypatch)
        runs.append((loc.grad.clone(), w.grad.clone() if aggregate else None))
    assert torch.equal(runs[0][0], runs[1][0])
    assert not aggregate or torch.equal(runs[0][1], runs[1][1])
