"""Autograd through BEVSampling's fused path without a GPU.

The two HIP launchers (bev_sampling_fused, bev_sampling_backward) are replaced HERE by the float64 torch fakes of
tests/bev_sampling_ref.py, which behave like the real ones: plain tensors in and out, no autograd history, the backward
writing into the destinations it is handed.  What is checked is the host-side plumbing around them -- the four Linears, the
box table as a differentiable input, the value stream's torch branch, the B > 1 route through forward_unfused -- against the
reference's own autograd (tests/golden/bev_sampling_grad_small*.npz, gen_golden_bev_sampling_grad.py).  Also the closed-form
backward the kernel implements against float64 autograd, and the argument checks of rac_bev_sampling_bwd, which run before
any HIP call."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import bev_sampling_ref as BR
from oracle import restate as R
from racformer_amd import _lib
from racformer_amd import synthetic as syn
from racformer_amd import transformer as T

E = 256


def t(a):
    return torch.from_numpy(np.asarray(a)).clone()


def load_golden(golden_dir):
    """the fixture is dealt over several files (each below the 1 MiB limit for a committed file)"""
    g = {}
    for path in sorted(glob.glob(os.path.join(golden_dir, "bev_sampling_grad_small*.npz"))):
        with np.load(path) as z:
            g.update({k: z[k] for k in z.files})
    assert "b1:out" in g and "b2:out" in g
    return g


def module_from(g, dtype=torch.float32, requires_grad=True):
    heads, Tn, NP, D, H, W = (int(x) for x in g["shape"])
    m = T.BEVSampling(embed_dims=E, num_frames=Tn, num_points=NP, num_heads=heads, num_levels=1, pc_range=list(syn.PC_RANGE),
                      spatial_shapes=(W, H), depth_num=D, temp_radar=False).eval()
    m.load_state_dict({k[2:]: t(v).float() for k, v in g.items() if k.startswith("w:")})
    m = m.to(dtype)
    for p in m.parameters():
        p.requires_grad_(requires_grad)
    return m


def inputs_from(g, pre, dtype=torch.float32):
    qr, qf, bev = (t(g[pre + k]).to(dtype).requires_grad_() for k in ("query_ray", "query_feat", "bev_feats"))
    return qr, qf, bev, [dict(time_diff=t(g[pre + "time_diff"]).to(dtype))], t(g[pre + "gout"]).to(dtype)


def rel_err(got, want):
    want = t(want).double()
    return ((got.detach().cpu().double() - want).abs().max() / want.abs().max()).item()


# The reference runs in float32 (MSDA through grid_sample, float32 softmaxes and trigonometry); the fakes in float64, the
# torch layers around them in float32.  Same kind of comparison and same tolerances as test_sasa_grad_cpu.py /
# test_mixing_grad_cpu.py: max |err| / max |value| per tensor.
TOL_OUT, TOL_GRAD = 5e-6, 1e-5


@pytest.fixture
def fakes(monkeypatch):
    monkeypatch.setattr(T, "bev_sampling_fused", BR.fake_fused)
    monkeypatch.setattr(T, "bev_sampling_backward", BR.fake_backward)
    BR.CALLS.clear()


def fake_msda_fwd(value, shapes, starts, loc, attn, out=None):
    with torch.no_grad():
        return R.msda_torch(value.double(), shapes, starts, loc.double(), attn.double()).to(value.dtype)


def fake_msda_bwd(grad, value, shapes, starts, loc, attn):
    with torch.enable_grad():
        v, lo, a = (x.detach().double().requires_grad_() for x in (value, loc, attn))
        got = torch.autograd.grad(R.msda_torch(v, shapes, starts, lo, a), (v, lo, a), grad.double())
    return tuple(x.detach().to(value.dtype) for x in got)


@pytest.fixture
def fake_msda(monkeypatch):
    monkeypatch.setattr(T, "msda_forward", fake_msda_fwd)
    monkeypatch.setattr(T, "msda_backward", fake_msda_bwd)


def check_against_golden(g, pre, m, qr, qf, bev, out):
    assert rel_err(out, g[pre + "out"]) < TOL_OUT
    worst = {}
    for name, got in [("query_feat", qf.grad), ("bev_feats", bev.grad), ("query_ray", qr.grad)] + \
            [(k, p.grad) for k, p in m.named_parameters()]:
        assert got is not None, f"{name}: no gradient"
        worst[name] = rel_err(got, g[pre + "g:" + name])
    print("\n" + "\n".join(f"  {k:>40s}: {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v < TOL_GRAD}
    assert not bad, bad
    gq = qr.grad
    assert float(gq[..., [2, 5, 8, 9]].abs().max()) == 0.0 and all(float(gq[..., i].abs().max()) > 0 for i in (0, 1, 3, 4, 6, 7))


def test_module_gradients_match_the_reference_b1(golden_dir, fakes):
    """every key of the golden through _BEVSamplingCore; fails where the fused path has no autograd history"""
    g = load_golden(golden_dir)
    m = module_from(g)
    qr, qf, bev, metas, gout = inputs_from(g, "b1:")
    out = m(qr, qf, bev, metas, d_region=float(g["d_region"]))
    (out * gout).sum().backward()
    assert [c[0] for c in BR.CALLS] == ["fwd", "bwd"]
    assert BR.CALLS[0][13] is False and BR.CALLS[1] == ("bwd", (1, 21, 256), True, False)   # no caller's table; contiguous grad
    check_against_golden(g, "b1:", m, qr, qf, bev, out)


def test_caller_table_and_linear_out_b1(golden_dir, fakes):
    """the decoder layer's way of calling: Linear outputs as column slices of one wide GEMM output, its own box table"""
    g = load_golden(golden_dir)
    m = module_from(g)
    qr, qf, bev, metas, gout = inputs_from(g, "b1:")
    mods = [m.sampling_offset, m.ray_points_offset, m.scale_weights, m.attention.bev_queue_weight]
    wide = torch.nn.functional.linear(qf, torch.cat([x.weight for x in mods]), torch.cat([x.bias for x in mods]))
    lin = wide.split([x.weight.shape[0] for x in mods], dim=-1)
    value, hw = m.prepare_value(bev)
    table = T.box_table_torch(qr.detach(), m.pc_range)
    out = m.attend_prepared(qr, qf, value, hw, metas[0]["time_diff"], float(g["d_region"]), linear_out=lin, box_table=table)
    (out * gout).sum().backward()
    assert BR.CALLS[0][13] is True and BR.CALLS[1][3] is True
    check_against_golden(g, "b1:", m, qr, qf, bev, out)


def test_module_gradients_match_the_reference_b2(golden_dir, fakes, fake_msda):
    """B = 2 takes forward_unfused (the reference's frame / batch pairing): neither fused launcher runs"""
    g = load_golden(golden_dir)
    m = module_from(g)
    qr, qf, bev, metas, gout = inputs_from(g, "b2:")
    out = m(qr, qf, bev, metas, d_region=float(g["d_region"]))
    (out * gout).sum().backward()
    assert BR.CALLS == []
    check_against_golden(g, "b2:", m, qr, qf, bev, out)


def test_no_grad_and_frozen_launch_what_they_launched_before(golden_dir, fakes):
    """under no_grad / inference_mode, and in grad mode with nothing requiring grad: one plain forward launch with today's arguments"""
    g = load_golden(golden_dir)
    m = module_from(g)
    qr, qf, bev, metas, _ = inputs_from(g, "b1:")
    d_region = float(g["d_region"])
    with torch.no_grad():
        a = m(qr, qf, bev, metas, d_region=d_region)
    with torch.inference_mode():
        b = m(qr, qf, bev, metas, d_region=d_region)
    c = module_from(g, requires_grad=False)(qr.detach(), qf.detach(), bev.detach(), metas, d_region=d_region)
    heads, Tn, NP, D, H, W = (int(x) for x in g["shape"])
    P = NP * D
    want = ("fwd", (Tn, H * W, heads, 64), (H, W), (1, 21, 10), heads * P * 2, D, heads * P, Tn, Tn, heads, NP, D, d_region, False,
            False, False)
    assert BR.CALLS == [want] * 3
    for o in (a, b, c):
        assert o.grad_fn is None and rel_err(o, g["b1:out"]) < TOL_OUT
    # B = 2 under no_grad still launches the fused forward (it reproduces the pairing itself)
    BR.CALLS.clear()
    qr2, qf2, bev2, metas2, _ = inputs_from(g, "b2:")
    with torch.no_grad(), pytest.raises(AssertionError):      # (the float64 fake restates B == 1 only: reaching it is the point)
        m(qr2, qf2, bev2, metas2, d_region=d_region)
    assert [c_[0] for c_ in BR.CALLS] == ["fwd"]


def test_prepare_value_under_grad_takes_the_torch_branch(golden_dir):
    """a packed convolution has no autograd history: with a pack, the value stream still carries its gradient"""
    m = T.BEVSampling(embed_dims=E, num_frames=2, num_points=1, num_heads=4, num_levels=1, pc_range=list(syn.PC_RANGE),
                      spatial_shapes=(4, 4), depth_num=2, temp_radar=True).eval()
    bev = torch.randn(1, 2, E, 4, 4)
    pack = dict(ws=object())                                    # never touched on the torch branch
    value, hw = m.prepare_value(bev, pack)
    assert value.grad_fn is not None and hw == (4, 4)
    for p in m.parameters():
        p.requires_grad_(False)
    assert m._value_needs_grad(bev) is False and m._value_needs_grad(bev.clone().requires_grad_()) is True
    with torch.no_grad():
        assert m._value_needs_grad(bev.clone().requires_grad_()) is False


# ------------------------------------------------------------------------------------------------------ the closed form
def _case(seed, Q, heads, Tn, NP, D, H, W, outside=False):
    rng = np.random.default_rng(seed)
    P = NP * D
    qb = t(rng.random((1, Q, 10)))
    qb[..., 1] = 0.05 + 0.55 * qb[..., 1]
    if outside:
        qb[:, ::2, 1] = 1.3                                     # far outside the map: clamped keypoints
    qb[..., 6:8] = qb[..., 6:8] * 2 - 1
    qb[..., 8:10] = qb[..., 8:10] * 4 - 2
    return dict(value=t(rng.standard_normal((Tn, H * W, heads, 64))), hw=(H, W), query_bbox=qb,
                off=t(rng.uniform(-1.5, 1.5, (1, Q, heads * P * 2))), ray=t(rng.standard_normal((1, Q, D))),
                sc=t(rng.standard_normal((1, Q, heads * P))), qu=t(rng.standard_normal((1, Q, Tn))),
                time_diff=t(rng.random((1, Tn)) + np.arange(Tn) * 0.5), T=Tn, heads=heads, NP=NP, D=D, pc=list(syn.PC_RANGE),
                d_region=0.1), t(rng.standard_normal((1, Q, heads * 64)))


@pytest.mark.parametrize("shape", [(5, 4, 3, 2, 5, 12, 10, False), (4, 3, 1, 1, 3, 8, 8, False), (6, 1, 8, 3, 2, 16, 16, True)])
def test_closed_form_backward_is_the_autograd_of_the_chain(shape):
    """every output of rac_bev_sampling_bwd's table, formula by formula, against float64 autograd: of the restated forward
    (core64, with the box table as an input) and of the module's own torch chain (forward_unfused: keypoints + MSDA + fusion)"""
    *dims, outside = shape
    c, gout = _case(sum(dims), *dims, outside=outside)
    Q, heads, Tn, NP, D, H, W = dims
    P = NP * D
    got = BR.closed_form_bwd(gout=gout, **c)
    # (a) autograd of core64 in the same inputs, the box table a leaf
    leaves = {k: c[k].clone().requires_grad_() for k in ("value", "off", "ray", "sc", "qu")}
    table = T.box_table_torch(c["query_bbox"], c["pc"]).requires_grad_()
    out, loc = BR.core64(**{**c, **leaves}, box_table=table)
    loc.retain_grad()
    (out * gout).sum().backward()
    want = dict(grad_value=leaves["value"].grad, grad_offsets=leaves["off"].grad, grad_ray=leaves["ray"].grad,
                grad_scale=leaves["sc"].grad, grad_queue=leaves["qu"].grad, grad_box=table.grad, grad_loc=loc.grad)
    if outside:
        assert bool(((loc == 0) | (loc == 1)).any())
    for k, w_ in want.items():
        assert (got[k] - w_).abs().max().item() < 1e-11 * max(1.0, w_.abs().max().item()), k
    assert float(got["grad_box"][..., [2, 5]].abs().max()) == 0.0
    # grad_attn: d out / d (aw * qw) per keypoint
    smp = BR.sampled64(c["value"], loc.detach()[0], c["hw"])
    assert (got["grad_attn"][0] - (smp * gout.reshape(Q, heads, 1, 1, 64)).sum(-1)).abs().max().item() < 1e-11
    # (b) the module's torch chain: same output, same gradients (grad_box carried on to query_ray by plain autograd)
    m = T.BEVSampling(embed_dims=heads * 64, num_frames=Tn, num_points=NP, num_heads=heads, num_levels=1, pc_range=c["pc"],
                      spatial_shapes=(W, H), depth_num=D).double()
    m.attention.num_heads = heads
    qr = c["query_bbox"].clone().requires_grad_()
    lv = {k: c[k].clone().requires_grad_() for k in ("off", "ray", "sc", "qu")}
    kloc, sw = m.keypoints(qr, torch.zeros(1, Q, heads * 64, dtype=torch.float64), c["time_diff"], c["d_region"],
                           (lv["off"], lv["ray"], lv["sc"]))
    # (the launcher's depth bases are float32 numbers, linspace(-d_region, d_region, D) as the reference forms them on the host;
    # the module's float64 chain forms them in float64: 1.5e-9 apart, which is what these comparisons allow for)
    assert (kloc - loc.detach()).abs().max().item() < 1e-8
    qw = torch.softmax(lv["qu"], -1)
    out2 = (BR.sampled64(c["value"], kloc[0], c["hw"]) * (sw[0, :, :, :, 0, :] * qw[0][:, None, :, None])[..., None]).sum((2, 3))
    assert (out2.reshape(1, Q, -1) - out.detach()).abs().max().item() < 1e-6
    (out2.reshape(1, Q, -1) * gout).sum().backward()
    table2 = T.box_table_torch(qr2 := c["query_bbox"].clone().requires_grad_(), c["pc"])
    table2.backward(got["grad_box"])
    for a, b in ((got["grad_offsets"], lv["off"].grad), (got["grad_ray"], lv["ray"].grad), (got["grad_scale"], lv["sc"].grad),
                 (got["grad_queue"], lv["qu"].grad), (qr2.grad, qr.grad)):
        assert (a - b).abs().max().item() < 1e-6 * max(1.0, b.abs().max().item())
    assert float(qr.grad[..., [2, 5, 8, 9]].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------ argument checks
def _lib_or_fail():
    try:
        return _lib.lib()
    except RuntimeError as e:
        pytest.fail(str(e))


def test_bev_sampling_bwd_argument_errors():
    lib = _lib_or_fail()
    d = ctypes.c_void_p(16)                     # never dereferenced: every failing call below fails its checks first
    pc = (ctypes.c_float * 6)(*syn.PC_RANGE)
    db = (ctypes.c_float * 5)(-0.1, -0.05, 0.0, 0.05, 0.1)

    def last():
        return lib.rac_last_error().decode()

    def bwd(B=1, Tn=3, Q=21, heads=4, NP=2, D=5, H=12, W=10, dim=64, dtype=_lib.RAC_F32, ld=(80, 5, 40, 3), gld=(80, 5, 40, 3),
            ptr=d, gv=d, host=True):
        return lib.rac_bev_sampling_bwd(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, gv, ptr, ptr, ptr, ptr, ptr, None, None,
                                        *ld, *gld, B, Tn, Q, heads, NP, D, H, W, dim, pc if host else None, db if host else None,
                                        0.1, dtype, None)

    assert bwd(B=2) == -1 and "B=2" in last() and "rac_bev_sampling_bwd" in last()
    assert bwd(dtype=_lib.RAC_BF16) == -1 and "dtype 1" in last()
    assert bwd(dtype=_lib.RAC_I16) == -1 and "dtype 2" in last()
    assert bwd(dim=32) == -1 and "dim=32" in last()
    assert bwd(D=17) == -1 and "bad sizes" in last()
    assert bwd(Tn=0) == -1 and "bad sizes" in last()
    assert bwd(Tn=65) == -1 and "max 64" in last()
    assert bwd(NP=13) == -1 and "max 64" in last()                        # 13 * 5 points
    assert bwd(ld=(79, 5, 40, 3)) == -1 and "row strides" in last()
    assert bwd(ld=(80, 5, 40, 2)) == -1 and "row strides" in last()
    assert bwd(gld=(80, 4, 40, 3)) == -1 and "gradient row strides" in last()
    assert bwd(gld=(80, 5, 39, 3)) == -1 and "gradient row strides" in last()
    assert bwd(heads=16, Tn=64, NP=2, D=5, ld=(320, 5, 160, 64), gld=(320, 5, 160, 64)) == -1 and "LDS staging" in last()
    assert bwd(ptr=None) == -1 and "null pointer" in last()
    assert bwd(gv=None) == -1 and "null pointer" in last()
    assert bwd(host=False) == -1 and "null pointer" in last()
    assert bwd(Q=0, ptr=None, gv=None) == 0 and bwd(B=0, ptr=None, gv=None) == 0     # empty: nothing to check or launch
