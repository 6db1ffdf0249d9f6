"""Autograd through sampling_4d (both modes) and BEVSelfAttention without a GPU.

The HIP launchers are replaced HERE, in the test, by oracle-backed fakes that behave like the real ones: the forwards and
the backwards take and return plain tensors without autograd history, in the layouts the real ones use (the forward writes
[B,Q,G,T*P,C], the backward reads the gradient in that layout).  What is checked is the host-side plumbing around them --
the autograd Functions, the torch projection / selection ops and the weight-slot order -- against the reference's own
autograd (tests/golden/sampling4d_grad_small.npz, gen_golden_grad4d.py) and against a float64 composition of the oracle.
Also the argument checks of rac_msmv_bwd_ex / rac_msmv_v2_bwd_ex, which run before any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import restate as R
from racformer_amd import _lib
from racformer_amd import transformer as T


def t(a):
    return torch.from_numpy(np.asarray(a)).clone()


def to_bqgtpc(o, num_frames, num_groups):
    """[S,Q,C,P] with s = (b*T + t)*G + g -> [B,Q,G,T*P,C]"""
    S, Q, C, P = o.shape
    B = S // (num_frames * num_groups)
    return o.reshape(B, num_frames, num_groups, Q, C, P).permute(0, 3, 2, 1, 5, 4).reshape(B, Q, num_groups, num_frames * P, C)


def to_sqcp(x, num_frames, num_groups):
    """the inverse of to_bqgtpc"""
    B, Q, G, TP, C = x.shape
    P = TP // num_frames
    return x.reshape(B, Q, G, num_frames, P, C).permute(0, 3, 2, 1, 5, 4).reshape(B * num_frames * G, Q, C, P)


def onehot_argmax(w):
    return torch.nn.functional.one_hot(torch.argmax(w, dim=-1), w.shape[-1]).to(w.dtype)


# ----------------------------------------------------------------------------------- fakes of the four msmv launchers
def fake_fwd(feats, loc, w, out_layout=_lib.OUT_SQCP, num_frames=1, num_groups=1, out=None):
    with torch.no_grad():
        o = R.msmv_gather_torch(list(feats), loc, w)
    return to_bqgtpc(o, num_frames, num_groups).contiguous() if out_layout == _lib.OUT_BQGTPC else o


def fake_v2_fwd(feats, loc, w, out_layout=_lib.OUT_SQCP, num_frames=1, num_groups=1, channels_first=False, out=None):
    assert not channels_first
    return fake_fwd(feats, loc, onehot_argmax(w), out_layout, num_frames, num_groups)


CALLS = []


def _oracle_grads(grad, feats, loc, w, grad_layout, num_frames, num_groups, with_w):
    CALLS.append((grad_layout, num_frames, num_groups, tuple(grad.shape), grad.is_contiguous()))
    g = to_sqcp(grad, num_frames, num_groups) if grad_layout == _lib.OUT_BQGTPC else grad
    with torch.enable_grad():
        f = [x.detach().requires_grad_() for x in feats]
        lo = loc.detach().requires_grad_()
        ww = w.detach().requires_grad_(with_w)
        out = R.msmv_gather_torch(f, lo, ww if with_w else onehot_argmax(ww))
        got = torch.autograd.grad(out, f + [lo] + ([ww] if with_w else []), g)
    return [x.detach() for x in got]


def fake_bwd(grad, feats, loc, w, grad_layout=_lib.OUT_SQCP, num_frames=1, num_groups=1):
    *gf, gl, gw = _oracle_grads(grad, feats, loc, w, grad_layout, num_frames, num_groups, True)
    return gf, gl, gw


def fake_v2_bwd(grad, feats, loc, w, channels_first=False, grad_layout=_lib.OUT_SQCP, num_frames=1, num_groups=1):
    *gf, gl = _oracle_grads(grad, feats, loc, w, grad_layout, num_frames, num_groups, False)
    return gf, gl


@pytest.fixture
def fake_msmv(monkeypatch):
    monkeypatch.setattr(T, "msmv_forward", fake_fwd)
    monkeypatch.setattr(T, "msmv_v2_forward", fake_v2_fwd)
    monkeypatch.setattr(T, "msmv_backward", fake_bwd)
    monkeypatch.setattr(T, "msmv_v2_backward", fake_v2_bwd)
    CALLS.clear()


def _golden_inputs(g, pre):
    H, W = (int(x) for x in g[pre + "image_hw"])
    L = sum(1 for k in g.files if k.startswith(pre + "feat"))
    feats = [t(g[f"{pre}feat{i}"]).requires_grad_() for i in range(L)]
    pts = t(g[pre + "pts"]).requires_grad_()
    sw = t(g[pre + "scale_weights"]).requires_grad_()
    return pts, feats, sw, t(g[pre + "lidar2img"]), H, W


def _max_err(got, want):
    return (got - t(want)).abs().max().item()


# The reference's gradients come from grid_sample on [B', C, N, H, W] after a matmul projection; the fakes compute the
# kernel semantics in float32 after this package's own projection (explicit products and sums).  Tolerances: those of
# tests/test_backward.py for the operator-level golden (feature / weight gradients 2e-5, location gradients 2e-4), and for
# sample_points the location tolerance carried through the projection.  Each point is projected once (its own frame, the
# selected camera), so its gradient is grad_u * du/dx + grad_v * dv/dx (likewise y, z); over the points some camera sees in
# these fixtures |d(u|v)/d(x|y|z)| <= 0.5 (the nearest ones are a few metres from a camera with f = 140 px on a 176 x 64
# image), so an error of 2e-4 in each location gradient moves a point gradient by at most 2e-4 -- SCALE = 4 leaves a
# factor of 4 for the rounding of the projection chain itself.  Points no camera sees get zero location gradients from the
# kernel and from grid_sample alike.  Measured worst errors: feature 5e-7, weight 4e-6, point 3e-6.
TOL = {"feat": 2e-5, "w": 2e-5, "loc": 2e-4}
SCALE = 4.0


@pytest.mark.parametrize("pre", ["l4_", "l5_"])
@pytest.mark.parametrize("aggregate", [True, False])
def test_sampling_4d_gradients_match_the_reference(golden_dir, fake_msmv, pre, aggregate):
    g = np.load(os.path.join(golden_dir, "sampling4d_grad_small.npz"))
    mode = "agg_" if aggregate else "hard_"
    pts, feats, sw, l2i, H, W = _golden_inputs(g, pre)
    res = T.sampling_4d(pts, feats, sw, l2i, H, W, aggregate=aggregate)
    final = res if aggregate else res[0]
    assert final.requires_grad and final.grad_fn is not None
    assert _max_err(final.detach(), g[pre + mode + "final"]) < 2e-5
    (final * t(g[pre + "gout"])).sum().backward()
    B, Q, Tf, G, P, _ = pts.shape
    # one backward launch, handed the gradient in the forward's own layout, contiguous, no permute
    assert CALLS == [(_lib.OUT_BQGTPC, Tf, G, tuple(final.shape), True)]
    for i, f in enumerate(feats):
        assert _max_err(f.grad, g[f"{pre}{mode}gfeat{i}"]) < TOL["feat"], i
    if aggregate:
        assert _max_err(sw.grad, g[pre + mode + "gsw"]) < TOL["w"]
    else:
        assert sw.grad is None                                   # argmax: no weight gradient, as the reference
    assert not torch.isnan(pts.grad).any()
    assert _max_err(pts.grad, g[pre + mode + "gpts"]) < TOL["loc"] * SCALE
    assert pts.grad.abs().max().item() > 1.0                     # (the comparison is not between zeros)


def test_fixture_covers_the_edges(golden_dir):
    """points visible in no camera, points within a pixel of an image edge on both sides, B = 2, T*G > 1"""
    g = np.load(os.path.join(golden_dir, "sampling4d_grad_small.npz"))
    for pre in ("l4_", "l5_"):
        pts = t(g[pre + "pts"])
        B, Q, Tf, G, P, _ = pts.shape
        assert B == 2 and Tf * G > 1
        H, W = (int(x) for x in g[pre + "image_hw"])
        loc, _, seen = R.project_select(pts.reshape(B, Q, Tf, G * P, 3), t(g[pre + "lidar2img"]), H, W)
        assert not bool(seen.all())
        u, v = loc[..., 0], loc[..., 1]
        near = ((u - 1).abs() < 1e-3) | (u.abs() < 1e-3) | ((v - 1).abs() < 1e-3) | (v.abs() < 1e-3)
        assert bool((near & ((u > 1) | (u < 0) | (v > 1) | (v < 0))).any()) and bool((near & seen).any())


# ----------------------------------------------------------------------------------------------- BEVSelfAttention
def fake_msda_fwd(value, shapes, starts, loc, attn, out=None):
    with torch.no_grad():
        return R.msda_torch(value, shapes, starts, loc, attn)


MSDA_CALLS = []


def fake_msda_bwd(grad, value, shapes, starts, loc, attn):
    MSDA_CALLS.append(tuple(grad.shape))
    with torch.enable_grad():
        v, lo, a = (x.detach().requires_grad_() for x in (value, loc, attn))
        got = torch.autograd.grad(R.msda_torch(v, shapes, starts, lo, a), (v, lo, a), grad)
    return tuple(x.detach() for x in got)


def _bev_case(seed=7, B=2, Q=5, C=32, heads=4, Tq=3, P=6, H=5, W=7):
    g = torch.Generator().manual_seed(seed)
    mod = T.BEVSelfAttention(embed_dims=C, num_heads=heads, num_levels=1, num_points=P, num_bev_queue=Tq, queue_weight=True)
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.2)
    query = torch.randn(B, Q, C, generator=g)
    maps = torch.randn(B, Tq, C, H, W, generator=g)
    loc = torch.rand(B, Q, heads, Tq, P, 2, generator=g) * 1.2 - 0.1
    aw = torch.rand(B, Q, heads, Tq, 1, P, generator=g)
    return mod, query, maps, loc, aw, (H, W)


def test_bev_self_attention_gradients(monkeypatch):
    """every parameter and input gradient of BEVSelfAttention.forward against a float64 composition of the oracle's
    bev_self_attention (quirk Q2: locations / weights frame-major, values batch-major, as written) with msda_torch"""
    monkeypatch.setattr(T, "msda_forward", fake_msda_fwd)
    monkeypatch.setattr(T, "msda_backward", fake_msda_bwd)
    MSDA_CALLS.clear()
    mod, query, maps, loc, aw, hw = _bev_case()
    ins = [x.clone().requires_grad_() for x in (query, maps, loc, aw)]
    out = mod(ins[0], ins[1], ins[2], ins[3], spatial_shapes=hw)
    assert out.grad_fn is not None
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(3))
    (out * gout).sum().backward()
    assert len(MSDA_CALLS) == 1
    # float64 reference
    sd = {k: v.detach().double().requires_grad_() for k, v in mod.state_dict().items()}
    ref_ins = [x.detach().double().requires_grad_() for x in (query, maps, loc, aw)]
    monkeypatch.setattr(R, "msda", lambda *a: R.msda_torch(*a))
    ref = R.bev_self_attention({"m." + k: v for k, v in sd.items()}, "m", *ref_ins, heads=mod.num_heads)
    assert (out.detach().double() - ref.detach()).abs().max().item() < 1e-4
    (ref * gout.double()).sum().backward()
    named = [("query", ins[0], ref_ins[0]), ("value maps", ins[1], ref_ins[1]), ("sampling_locations", ins[2], ref_ins[2]),
             ("attention_weights", ins[3], ref_ins[3])]
    named += [(k, p, sd[k]) for k, p in mod.named_parameters()]
    assert {k for k, _ in mod.named_parameters()} == set(sd)      # value_proj, output_proj, bev_queue_weight
    for name, got, want in named:
        assert got.grad is not None, name
        scale = want.grad.abs().max().item()
        assert scale > 0, name
        err = (got.grad.double() - want.grad).abs().max().item()
        assert err <= 2e-5 * max(scale, 1.0), (name, err, scale)


# ----------------------------------------------------------------------------------------------- C entry points
def _lib_or_fail():
    try:
        return _lib.lib()
    except RuntimeError as e:
        pytest.fail(str(e))


def test_bwd_ex_argument_errors():
    lib = _lib_or_fail()
    dummy = ctypes.c_void_p(16)                     # never dereferenced: every failing call below fails its checks first
    feats = (ctypes.c_void_p * 2)(16, 16)
    gfeats = (ctypes.c_void_p * 2)(32, 32)
    hw = (ctypes.c_int32 * 4)(4, 6, 2, 3)

    def last():
        return lib.rac_last_error().decode()

    def v1(layout=_lib.OUT_BQGTPC, T_=2, G=3, S=12, Q=4, P=5, C=64, gout=dummy):
        return lib.rac_msmv_bwd_ex(gout, layout, T_, G, feats, hw, 2, dummy, dummy, gfeats, dummy, dummy, S, 3, Q, P, C, None)

    def v2(layout=_lib.OUT_BQGTPC, T_=2, G=3, S=12, Q=4, P=5, C=64, gout=dummy):
        return lib.rac_msmv_v2_bwd_ex(gout, layout, T_, G, feats, hw, 2, dummy, dummy, gfeats, dummy, S, 3, Q, P, C,
                                      _lib.FEAT_CL, None)

    for fn, name in ((v1, "rac_msmv_bwd_ex"), (v2, "rac_msmv_v2_bwd_ex")):
        assert fn(layout=2) == -1 and "gradient layout 2" in last() and name in last()
        assert fn(layout=-1) == -1 and "gradient layout" in last()
        assert fn(T_=0) == -1 and "T=0" in last()
        assert fn(G=0) == -1 and "G=0" in last()
        assert fn(layout=_lib.OUT_SQCP, T_=0) == -1                # T, G >= 1 in every layout
        assert fn(S=10) == -1 and "multiple of T*G" in last()
        assert fn(S=10, layout=_lib.OUT_SQCP, T_=1, G=1, gout=None) == -1 and "null" in last()   # SQCP: any S
        assert fn(S=0, gout=None) == 0                               # empty: nothing to check further or launch
        assert fn(gout=None) == -1 and "null" in last()              # a valid BQGTPC call gets as far as the pointers
    # the entry points without _ex keep their names in their errors
    assert lib.rac_msmv_bwd(None, feats, hw, 2, dummy, dummy, gfeats, dummy, dummy, 2, 3, 4, 5, 64, None) == -1
    assert last().startswith("rac_msmv_bwd:")
    assert lib.rac_msmv_v2_bwd(None, feats, hw, 2, dummy, dummy, gfeats, dummy, 2, 3, 4, 5, 64, _lib.FEAT_CL, None) == -1
    assert last().startswith("rac_msmv_v2_bwd:")
