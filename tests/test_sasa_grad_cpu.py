"""Autograd through ScaleAdaptiveSelfAttention's fused path without a GPU.

The two HIP launchers (sasa_fused with lse_out, sasa_backward) are replaced HERE, in the test, by float64 torch fakes that
behave like the real ones: plain tensors in and out, no autograd history, the backward writing into the destinations it is
handed.  What is checked is the host-side plumbing around them -- the slicing of the in_proj + gen_tau output ``lin``, the
leading dimensions, the one [B,Q,3E+heads] gradient buffer, the prepared-operand rule, no gradient for the boxes -- against
the reference's own autograd (tests/golden/sasa_grad_small.npz, gen_golden_sasa_grad.py).  Also the closed-form backward
the kernel implements against float64 autograd of the core, and the argument checks of rac_sasa_fwd_ex / rac_sasa_bwd,
which run before any HIP call."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from racformer_amd import _lib
from racformer_amd import synthetic as syn
from racformer_amd import transformer as T
from sasa_ref import _dist, _split, closed_form_bwd, core64

E, H = 128, 4
KEYS = ["attention.attn.in_proj_weight", "attention.attn.in_proj_bias", "attention.attn.out_proj.weight",
        "attention.attn.out_proj.bias", "gen_tau.weight", "gen_tau.bias"]


def t(a):
    return torch.from_numpy(np.asarray(a)).clone()


# ----------------------------------------------------------------------------------- fakes of the two launchers
CALLS = []


def fake_fused(qkv, tau, query_bbox, num_heads, pc_range, box_table=None, lse_out=None):
    CALLS.append(("fwd", lse_out is not None, qkv.shape[-1], qkv.stride(-2), tau.shape[-1], tau.stride(-2),
                  tau.data_ptr() - qkv.data_ptr()))
    with torch.no_grad():
        o, lse = core64(qkv, tau, query_bbox, num_heads, pc_range)
    if lse_out is not None:
        assert tuple(lse_out.shape) == tuple(lse.shape) and lse_out.is_contiguous()
        lse_out.copy_(lse)
    return o.float()


def fake_backward(qkv, tau, query_bbox, num_heads, pc_range, out, lse, grad_out, box_table=None, grad_qkv=None, grad_tau=None):
    CALLS.append(("bwd", qkv.stride(-2), grad_qkv.stride(-2), grad_tau.stride(-2), grad_tau.data_ptr() - grad_qkv.data_ptr(),
                  grad_out.is_contiguous(), query_bbox.requires_grad))
    with torch.no_grad():
        gq, gt = closed_form_bwd(qkv, tau, query_bbox, num_heads, pc_range, out, lse, grad_out)
    grad_qkv.copy_(gq)
    grad_tau.copy_(gt)
    return grad_qkv, grad_tau


@pytest.fixture
def fake_sasa(monkeypatch):
    monkeypatch.setattr(T, "sasa_fused", fake_fused)
    monkeypatch.setattr(T, "sasa_backward", fake_backward)
    CALLS.clear()


def _module(g, requires_grad=True):
    m = T.ScaleAdaptiveSelfAttention(embed_dims=E, num_heads=H, pc_range=syn.PC_RANGE).eval()
    m.load_state_dict({k: t(g["w:" + k]) for k in KEYS})
    for p in m.parameters():
        p.requires_grad_(requires_grad)
    return m


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "sasa_grad_small.npz"))


def _rel_err(got, want):
    want = t(want).double()
    return ((got.detach().double() - want).abs().max() / want.abs().max()).item()


# The fakes run the core in float64, the reference in float32 (logits up to O(1000) on the large-tau head): measured worst
# relative error (max |err| / max |value| per tensor) 6.7e-7 for the output, 2.2e-6 for a gradient (gen_tau.bias).
TOL_OUT, TOL_GRAD = 5e-6, 1e-5
WIDE = 3 * E + H     # 388 floats: q|k|v|tau of one token


@pytest.mark.parametrize("prepared", [None, "cached", "live"])
def test_module_gradients_match_the_reference(golden_dir, fake_sasa, prepared):
    """prepared: no operand / the decoder layer's cached operand (built under no_grad: must not cut the weight gradients) /
    an operand with autograd history (used as given)"""
    g = _golden(golden_dir)
    m = _module(g)
    qb = t(g["query_bbox"]).requires_grad_()
    qf = t(g["query_feat"]).requires_grad_()
    pw = None
    if prepared == "cached":
        with torch.no_grad():
            pw = m.wide_in_proj()
    elif prepared == "live":
        pw = m.wide_in_proj()
    out = m(qb, qf, None, pw)
    assert _rel_err(out, g["out"]) < TOL_OUT
    (out * t(g["gout"])).sum().backward()
    # one forward that saves the statistics, one backward; both read lin (388 wide) and the backward writes one 388-wide buffer
    B, Q, _ = qf.shape
    assert CALLS == [("fwd", True, 3 * E, WIDE, H, WIDE, 3 * E * 4), ("bwd", WIDE, WIDE, WIDE, 3 * E * 4, True, False)]
    assert _rel_err(qf.grad, g["g:query_feat"]) < TOL_GRAD
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        assert _rel_err(p.grad, g["g:" + k]) < TOL_GRAD, k
    assert qb.grad is None


def test_frozen_weights_query_gradient_only(golden_dir, fake_sasa):
    g = _golden(golden_dir)
    m = _module(g, requires_grad=False)
    qf = t(g["query_feat"]).requires_grad_()
    (m(t(g["query_bbox"]), qf, None) * t(g["gout"])).sum().backward()
    assert [c[0] for c in CALLS] == ["fwd", "bwd"]
    assert _rel_err(qf.grad, g["g:query_feat"]) < TOL_GRAD
    assert all(p.grad is None for p in m.parameters())


def test_no_grad_and_inference_run_the_plain_forward(golden_dir, fake_sasa):
    """no lse write, no autograd Function: what runs in the benchmark and the decoder plans"""
    g = _golden(golden_dir)
    m = _module(g)
    qb, qf = t(g["query_bbox"]), t(g["query_feat"])
    with torch.no_grad():
        a = m(qb, qf, None)
    with torch.inference_mode():
        b = m(qb, qf, None)
    m_frozen = _module(g, requires_grad=False)
    c = m_frozen(qb, qf, None)                     # grad mode, but nothing requires grad
    assert [x[:2] for x in CALLS] == [("fwd", False)] * 3
    for o in (a, b, c):
        assert o.grad_fn is None and _rel_err(o, g["out"]) < TOL_OUT


def test_golden_covers_the_edges(golden_dir):
    """tau = 0 exactly on one head, a negative and a large tau; coincident centres; rows almost one-hot"""
    g = _golden(golden_dir)
    qf = t(g["query_feat"]).double()
    tau = qf @ t(g["w:gen_tau.weight"]).double().t() + t(g["w:gen_tau.bias"]).double()
    assert bool((tau[..., 0] == 0).all()) and bool((tau[..., 2] < 0).any()) and float(tau[..., 3].min()) > 30
    r = _dist(t(g["query_bbox"]), syn.PC_RANGE)
    off_diag = ~torch.eye(r.shape[-1], dtype=torch.bool)
    assert bool((r[:, off_diag] == 0).any())
    m = T.ScaleAdaptiveSelfAttention(embed_dims=E, num_heads=H, pc_range=syn.PC_RANGE)
    m.load_state_dict({k: t(g["w:" + k]) for k in KEYS})
    with torch.no_grad():
        lin = torch.nn.functional.linear(qf.float(), *m.wide_in_proj())
        q, k, _ = _split(lin[..., :3 * E], H)
        s = q @ k.transpose(-1, -2) / math.sqrt(32) - r[:, None] * lin[..., 3 * E:].double().permute(0, 2, 1)[..., None]
        pmax = torch.softmax(s, dim=-1).max(-1).values          # [B,H,Q]
    assert float(pmax[:, 3].median()) > 0.99 and float(pmax[:, 0].median()) < 0.9    # one-hot rows and soft rows


@pytest.mark.parametrize("Q", [1, 17, 40])
def test_closed_form_backward_is_the_autograd_of_the_core(Q):
    """the formulas rac_sasa_bwd implements (dS = P o (dP - D), dq, dk, dv, dtau) against float64 autograd"""
    rng = np.random.default_rng(Q)
    B, Hn = 2, 3
    qkv = t(rng.standard_normal((B, Q, 3 * Hn * 32))).double().requires_grad_()
    tau = t(rng.random((B, Q, Hn)) * 2).double().requires_grad_()
    qb = t(rng.random((B, Q, 10)))
    if Q > 3:
        qb[:, 3] = qb[:, 1]
    gout = t(rng.standard_normal((B, Q, Hn * 32))).double()
    out, lse = core64(qkv, tau, qb, Hn, syn.PC_RANGE)
    want = torch.autograd.grad((out * gout).sum(), [qkv, tau])
    got = closed_form_bwd(qkv.detach(), tau.detach(), qb, Hn, syn.PC_RANGE, out.detach(), lse.detach(), gout)
    for a, b in zip(got, want):
        assert (a - b).abs().max().item() < 1e-12 * max(1.0, b.abs().max().item())


def _lib_or_fail():
    try:
        return _lib.lib()
    except RuntimeError as e:
        pytest.fail(str(e))


def test_sasa_argument_errors():
    lib = _lib_or_fail()
    d = ctypes.c_void_p(16)                     # never dereferenced: every failing call below fails its checks first
    pc = (ctypes.c_float * 6)(*syn.PC_RANGE)

    def last():
        return lib.rac_last_error().decode()

    def bwd(B=1, Q=37, heads=4, dim=32, ld_qkv=WIDE, ld_tau=WIDE, ld_gqkv=WIDE, ld_gtau=WIDE, ptr=d, lse=d):
        return lib.rac_sasa_bwd(ptr, ptr, ptr, None, ptr, lse, ptr, ptr, ptr, ld_qkv, ld_tau, ld_gqkv, ld_gtau, B, Q, heads, dim,
                                pc, None)

    def fwd_ex(B=1, Q=37, heads=4, dim=32, ld_qkv=WIDE, ld_tau=WIDE, ptr=d, lse=d):
        return lib.rac_sasa_fwd_ex(ptr, ptr, ptr, None, ptr, lse, ld_qkv, ld_tau, B, Q, heads, dim, pc, None)

    assert bwd(dim=64) == -1 and "head dim 64" in last() and "rac_sasa_bwd" in last()
    assert bwd(dim=16) == -1 and "head dim 16" in last()
    assert bwd(Q=-1) == -1 and "bad sizes" in last()
    assert bwd(heads=0) == -1 and "bad sizes" in last()
    assert bwd(ld_qkv=194) == -1 and "bad sizes" in last()              # ld_qkv % 4
    assert bwd(ld_qkv=3 * 4 * 32 - 4) == -1 and "bad sizes" in last()  # narrower than q|k|v
    assert bwd(ld_gqkv=389) == -1 and "bad sizes" in last()             # odd gradient row stride
    assert bwd(ld_gqkv=3 * 4 * 32 - 2) == -1 and "bad sizes" in last()
    assert bwd(ld_gtau=3) == -1 and "bad sizes" in last()
    assert bwd(ld_tau=3) == -1 and "bad sizes" in last()
    assert bwd(Q=6145) == -1 and "LDS centre table" in last()
    assert bwd(lse=None) == -1 and "null pointer" in last()
    assert bwd(ptr=None) == -1 and "null pointer" in last()
    assert bwd(B=0, ptr=None, lse=None) == 0 and bwd(Q=0, ptr=None, lse=None) == 0   # empty: nothing to check or launch
    assert fwd_ex(dim=64) == -1 and "head dim 64" in last() and "rac_sasa_fwd_ex" in last()
    assert fwd_ex(ld_qkv=194) == -1 and "bad sizes" in last()
    assert fwd_ex(Q=6145) == -1 and "LDS centre table" in last()
    assert fwd_ex(ptr=None) == -1 and "null pointer" in last()
    assert fwd_ex(B=0, ptr=None, lse=None) == 0
    # rac_sasa_fwd keeps its signature and its checks (it forwards to rac_sasa_fwd_ex without lse)
    assert lib.rac_sasa_fwd(d, d, d, None, d, WIDE, WIDE, 1, 37, 4, 16, pc, None) == -1 and "head dim 16" in last()
