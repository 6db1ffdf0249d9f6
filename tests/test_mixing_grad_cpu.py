"""Autograd through AdaptiveMixing's fused path without a GPU.

The two HIP launchers (mixing_fused, mixing_backward) are replaced HERE, in the test, by float64 torch fakes that behave like
the real ones: plain tensors in and out, no autograd history.  fused_supported is forced on.  What is checked is the host-side
plumbing around them -- _MixingCore, the grad-mode condition, the prepared-operand rule for out_proj_split -- against the
reference's own autograd (tests/golden/mixing_grad_small.npz, gen_golden_mixing_grad.py).  Also the closed-form backward the
kernel implements against float64 autograd of the core, and the argument checks of rac_mixing_bwd, which run before any HIP
call."""
import ctypes
import os

import numpy as np
import pytest
import torch

from racformer_amd import _lib
from racformer_amd import transformer as T
from mixing_ref import closed_form_bwd, core64, forward64, min_margin

KEYS = ["parameter_generator.weight", "parameter_generator.bias", "out_proj.weight", "out_proj.bias"]


def t(a):
    return torch.from_numpy(np.asarray(a)).clone()


# ----------------------------------------------------------------------------------- fakes of the two launchers
CALLS = []


def fake_fused(x, params, in_points, n_groups, out_points=128, eps=1e-5, split=False, param_scale=1.0, f16x3=False, out=None):
    CALLS.append(("fwd", split, f16x3, param_scale, x.is_contiguous(), params.requires_grad))
    with torch.no_grad():
        return core64(x, params, in_points, n_groups).float()


def fake_backward(x, params, grad_out, in_points, n_groups, out_points=128, eps=1e-5, grad_x=None, grad_params=None, z_out=None):
    CALLS.append(("bwd", x.requires_grad, params.requires_grad, grad_out.is_contiguous(), tuple(grad_out.shape)))
    with torch.no_grad():
        gx, gp = closed_form_bwd(x, params, grad_out, in_points, n_groups)
    return gx.float(), gp.float()


SPLITS = []


@pytest.fixture
def fake_mixing(monkeypatch):
    monkeypatch.setattr(T, "mixing_fused", fake_fused)
    monkeypatch.setattr(T, "mixing_backward", fake_backward, raising=False)
    monkeypatch.setattr(T.AdaptiveMixing, "fused_supported", lambda self, x: True)
    real_split = T.AdaptiveMixing.split_out_proj

    def counted_split(self):
        SPLITS.append(torch.is_grad_enabled())
        return real_split(self)

    monkeypatch.setattr(T.AdaptiveMixing, "split_out_proj", counted_split)
    CALLS.clear()
    SPLITS.clear()


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mixing_grad_small.npz"))


def _module(g, requires_grad=True):
    P, G = int(g["in_points"]), int(g["n_groups"])
    QD = g["query"].shape[-1]
    m = T.AdaptiveMixing(in_dim=64 * G, in_points=P, n_groups=G, query_dim=QD, out_points=128).eval()
    m.load_state_dict({k: t(g["w:" + k]).float() for k in KEYS})
    for p in m.parameters():
        p.requires_grad_(requires_grad)
    return m


def _cached_split(m):
    with torch.no_grad():
        s = T.AdaptiveMixing.split_out_proj(m)
    SPLITS.clear()
    return s


def _rel_err(got, want):
    want = t(want).double()
    return ((got.detach().double() - want).abs().max() / want.abs().max()).item()


# The fakes run the core in float64, the reference in float32: measured worst relative error (max |err| / max |value| per
# tensor) 3.4e-7 for the output, 6.0e-7 for a gradient (x).
TOL_OUT, TOL_GRAD = 2e-6, 1e-5


@pytest.mark.parametrize("prepared", ["cached", "live"])
def test_module_gradients_match_the_reference(golden_dir, fake_mixing, prepared):
    """prepared: the decoder layer's cached out_proj_split (built under no_grad: must not cut out_proj's weight gradient, so it
    is rebuilt under grad) / an operand with autograd history (used as given).  Before _MixingCore the fused path returned a
    tensor without history: x and parameter_generator got no gradient."""
    g = _golden(golden_dir)
    m = _module(g)
    x = t(g["x"]).requires_grad_()
    query = t(g["query"]).requires_grad_()
    split = _cached_split(m) if prepared == "cached" else m.split_out_proj()
    SPLITS.clear()
    out = m(x, query, split)
    assert _rel_err(out, g["out"]) < TOL_OUT
    (out * t(g["gout"])).sum().backward()
    B, Q = x.shape[:2]
    assert CALLS == [("fwd", False, False, 1.0, True, True), ("bwd", True, True, True, (B, Q, 2 * 128 * 64))]
    assert SPLITS == ([True] if prepared == "cached" else [])
    for name, v in [("x", x.grad), ("query", query.grad)] + [(k, p.grad) for k, p in m.named_parameters()]:
        assert v is not None, f"{name}: no gradient"
        assert _rel_err(v, g["g:" + name]) < TOL_GRAD, name


def test_frozen_weights_input_gradients_only(golden_dir, fake_mixing):
    """weights frozen (out_proj.weight does not require grad: the cached operand is used as given), x and query trainable"""
    g = _golden(golden_dir)
    m = _module(g, requires_grad=False)
    x = t(g["x"]).requires_grad_()
    query = t(g["query"]).requires_grad_()
    (m(x, query, _cached_split(m)) * t(g["gout"])).sum().backward()
    assert [c[0] for c in CALLS] == ["fwd", "bwd"] and SPLITS == []
    assert _rel_err(x.grad, g["g:x"]) < TOL_GRAD
    assert _rel_err(query.grad, g["g:query"]) < TOL_GRAD
    assert all(p.grad is None for p in m.parameters())


def test_only_x_requires_grad(golden_dir, fake_mixing):
    g = _golden(golden_dir)
    m = _module(g, requires_grad=False)
    x = t(g["x"]).requires_grad_()
    (m(x, t(g["query"]), _cached_split(m)) * t(g["gout"])).sum().backward()
    assert [c[0] for c in CALLS] == ["fwd", "bwd"]
    assert _rel_err(x.grad, g["g:x"]) < TOL_GRAD


def test_no_grad_and_inference_run_the_plain_forward(golden_dir, fake_mixing):
    """no autograd Function and no rebuilt operand: what runs in the benchmark and the decoder plans"""
    g = _golden(golden_dir)
    m = _module(g)
    split = _cached_split(m)
    x, query = t(g["x"]), t(g["query"])
    with torch.no_grad():
        a = m(x, query, split)
    with torch.inference_mode():
        b = m(x, query, split)
    c = _module(g, requires_grad=False)(x, query, split)      # grad mode, but nothing requires grad
    assert [cl[:4] for cl in CALLS] == [("fwd", False, False, 1.0)] * 3 and SPLITS == []
    for o in (a, b, c):
        assert o.grad_fn is None and _rel_err(o, g["out"]) < TOL_OUT


def test_golden_covers_the_fused_shape(golden_dir):
    """P odd (unaligned S rows), two groups of 64 channels, 128 out points; pre-activations clear of zero on both sides"""
    g = _golden(golden_dir)
    P, G = int(g["in_points"]), int(g["n_groups"])
    assert P % 2 == 1 and G == 2 and g["x"].shape[-1] == 64
    m = _module(g)
    with torch.no_grad():
        params = m.parameter_generator(t(g["query"]))
        f = forward64(t(g["x"]), params, P, G)
    assert float(min_margin(t(g["x"]), params, P, G).min()) >= 2.0 ** -12
    assert bool((f["Ah"] > 0).any()) and bool((f["Ah"] < 0).any()) and bool((f["Bh"] > 0).any()) and bool((f["Bh"] < 0).any())


def _case(P, G, N, seed):
    rng = np.random.default_rng(seed)
    x = t(rng.standard_normal((1, N, G, P, 64)))
    params = t(rng.standard_normal((1, N, G * (4096 + 128 * P))) * 0.2)
    gout = t(rng.standard_normal((1, N, G * 128 * 64)))
    return x, params, gout


@pytest.mark.parametrize("P,G", [(1, 1), (7, 2), (13, 1), (16, 3)])
def test_closed_form_backward_is_the_autograd_of_the_core(P, G):
    """the formulas rac_mixing_bwd implements (ReLU masks > 0, LayerNorm backward, the four products) against float64
    autograd, including a zero-variance item in each LayerNorm (x = 0: A constant; S = 0: B constant)"""
    x, params, gout = _case(P, G, 3, seed=P * 10 + G)
    x[0, 1, 0] = 0.0
    params[0, 2, 4096:4096 + 128 * P] = 0.0
    x = x.double().requires_grad_()
    params = params.double().requires_grad_()
    want = torch.autograd.grad((core64(x, params, P, G) * gout).sum(), [x, params])
    got = closed_form_bwd(x.detach(), params.detach(), gout, P, G)
    for a, b in zip(got, want):
        assert a.shape == b.shape
        assert (a - b).abs().max().item() < 1e-12 * max(1.0, b.abs().max().item())
    assert float(got[0][0, 1, 0].abs().max()) == 0.0                   # all of item (1, g0) is masked: no gradient
    assert float(got[1][0, 2, 4096:4096 + 128 * P].abs().max()) == 0.0   # B = 0: no dS


def _lib_or_fail():
    try:
        return _lib.lib()
    except RuntimeError as e:
        pytest.fail(str(e))


def test_mixing_bwd_argument_errors():
    lib = _lib_or_fail()
    d = ctypes.c_void_p(16)                     # never dereferenced: every failing call below fails its checks first
    P, G = 13, 2
    W = G * (4096 + 128 * P)

    def last():
        return lib.rac_last_error().decode()

    def bwd(nq=5, G=G, P=P, C=64, out=128, ld=W, ld_g=W, ptr=d, gout=d, z=None):
        return lib.rac_mixing_bwd(ptr, ptr, ld, gout, ptr, ptr, ld_g, z, nq, G, P, C, out, 1e-5, None)

    assert bwd(C=32) == -1 and "64 channels" in last() and "rac_mixing_bwd" in last()
    assert bwd(out=64) == -1 and "128 out points" in last()
    assert bwd(P=0) == -1 and "in_points=0" in last()
    assert bwd(P=97, ld=2 * (4096 + 128 * 97), ld_g=2 * (4096 + 128 * 97)) == -1 and "in_points=97" in last()
    assert bwd(nq=-1) == -1 and "bad sizes" in last()
    assert bwd(G=0) == -1 and "bad sizes" in last()
    assert bwd(ld=W - 4) == -1 and "parameter row stride" in last()
    assert bwd(ld=W + 2) == -1 and "parameter row stride" in last()        # not a multiple of 4 (float4 staging)
    assert bwd(ld_g=W - 1) == -1 and "gradient row stride" in last()
    assert bwd(ptr=None) == -1 and "null pointer" in last()
    assert bwd(gout=None) == -1 and "null pointer" in last()
    assert bwd(nq=0, ptr=None, gout=None) == 0            # empty: nothing to check or launch
