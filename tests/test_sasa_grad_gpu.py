"""ScaleAdaptiveSelfAttention's fused path is differentiable on the MI355X: rac_sasa_fwd_ex (the forward plus each row's
log-sum-exp) and rac_sasa_bwd (dq, dk, dv, dtau; single writer per element, no atomics).

  * module gradients against the reference's own autograd (tests/golden/sasa_grad_small.npz, gen_golden_sasa_grad.py);
  * kernel gradients element by element against float64 (tests/sasa_ref.py) over both forward kernels' ranges of Q, B,
    with and without the box table, the strided 776-wide lin, tau = 0, a large tau and coincident centres, under the bound
    ``|got - ref| <= K[kind] * 2**-24 * A`` of tests/test_backward_f64_gpu.py (A: the same computation with non-negative
    terms; the worst err / A per kind is printed at the end of the module), with a negative control (one key dropped);
  * lse against float64 logsumexp; rac_sasa_fwd_ex's output bit-identical to rac_sasa_fwd's with and without lse;
  * bit-reproducible backward; the grad-mode module output bit-identical to the no_grad one;
  * at the f8 shape (B = 1, Q = 900, 8 heads) all module gradients against forward_unfused's autograd in float64."""
import ctypes
import os

import numpy as np
import pytest
import torch

from racformer_amd import _lib
from racformer_amd import synthetic as syn
from racformer_amd import transformer as T
from racformer_amd.fused import box_prep, sasa_backward, sasa_fused
from sasa_ref import reference_with_scales

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
# One factor per kind.  Every element is a sum of at most Q products of rounded factors, formed in a fixed order.
K = {"dq": 64.0, "dk": 64.0, "dv": 64.0, "dtau": 64.0, "lse": 64.0}
# Absolute floor: a probability below ~1e-45 is 0 in float32 (exp underflows); the terms it would carry are far below this.
# The worst err / A is reported over the elements whose relative bound K*2^-24*A is above the floor.
TINY = 1e-30
WORST = {}
KEYS = ["attention.attn.in_proj_weight", "attention.attn.in_proj_bias", "attention.attn.out_proj.weight",
        "attention.attn.out_proj.bias", "gen_tau.weight", "gen_tau.bias"]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst err/A per kind, in units of 2**-24 (bound K):")
    for name in sorted(WORST):
        print(f"  {name:>44s}: {WORST[name] / U:9.3f}   (K = {K[name.split(':')[0]]:g})")


def t(a):
    return torch.from_numpy(np.asarray(a)).clone()


def _bad(kind, got, ref, A):
    err = (got.double() - ref).abs()
    return err, ~(err <= K[kind] * U * A + TINY)


def check(name, kind, got, ref, A):
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite {kind} written"
    err, bad = _bad(kind, got, ref, A)
    pos = K[kind] * U * A > TINY
    key = f"{kind}:{name}"
    WORST[key] = max(WORST.get(key, 0.0), float((err[pos] / A[pos]).max()) if bool(pos.any()) else 0.0)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        pytest.fail(f"{name}: {int(bad.sum())} of {bad.numel()} {kind} outside {K[kind]:g}*2^-24*A; first at flat {i}: "
                    f"got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} A {float(A.flatten()[i])!r}")


def make_case(B, Q, H, seed, tau_mode="mixed", coincident=True):
    """lin [B,Q,W] (q|k|v|tau in the first 3*32*H + H columns of a row padded to a multiple of 4: 776 at H = 8), boxes, grad"""
    g = torch.Generator().manual_seed(seed)
    E = 32 * H
    W = (3 * E + H + 3) // 4 * 4
    lin = torch.randn(B, Q, W, generator=g) * 1.5
    tau = torch.rand(B, Q, H, generator=g) * 2
    if tau_mode == "mixed" and H >= 3:
        tau[..., 0] = 0.0           # tau = 0
        tau[..., 1] *= 20.0         # large tau: rows almost one-hot
    elif tau_mode == "zero":
        tau.zero_()
    elif tau_mode == "large":
        tau = tau * 30.0
    lin[..., 3 * E:3 * E + H] = tau
    qb = torch.rand(B, Q, 10, generator=g)
    if coincident and Q >= 8:
        qb[:, 5] = qb[:, 2]
        qb[:, Q - 1] = qb[:, 0]
    gout = torch.randn(B, Q, E, generator=g)
    return [x.to(DEV) for x in (lin, qb, gout)], E


def run_kernels(lin, qb, gout, H, E, table=None, wide_grad=True):
    qkv, tau = lin[..., :3 * E], lin[..., 3 * E:3 * E + H]
    B, Q, _ = qb.shape
    lse = torch.full((B, H, Q), float("nan"), device=DEV)
    out = sasa_fused(qkv, tau, qb, H, syn.PC_RANGE, box_table=table, lse_out=lse)
    if wide_grad:   # one buffer shaped like lin, pre-filled with NaN: every element of the two slices must be written
        buf = torch.full(lin.shape, float("nan"), device=DEV)
        gq, gt = buf[..., :3 * E], buf[..., 3 * E:3 * E + H]
    else:
        gq = torch.full((B, Q, 3 * E), float("nan"), device=DEV)
        gt = torch.full((B, Q, H), float("nan"), device=DEV)
    sasa_backward(qkv, tau, qb, H, syn.PC_RANGE, out, lse, gout, box_table=table, grad_qkv=gq, grad_tau=gt)
    torch.cuda.synchronize()
    return out, lse, gq, gt


def split_grads(gq, gt, E):
    return {"dq": gq[..., :E], "dk": gq[..., E:2 * E], "dv": gq[..., 2 * E:], "dtau": gt}


CASES = [  # (B, Q, heads, table, tau_mode, wide_grad)
    (4, 1, 4, False, "mixed", True), (4, 15, 4, True, "mixed", True), (2, 16, 4, False, "large", False),
    (4, 17, 4, True, "mixed", True), (2, 64, 8, False, "mixed", True), (1, 64, 8, True, "zero", True),
    (2, 900, 8, True, "mixed", True), (1, 1024, 4, False, "mixed", False), (2, 1100, 4, True, "mixed", True),
    (1, 2048, 3, False, "mixed", True), (1, 2048, 2, True, "large", True),
]


@pytest.mark.parametrize("B,Q,H,table,tau_mode,wide", CASES)
def test_kernel_gradients_against_float64(B, Q, H, table, tau_mode, wide):
    (lin, qb, gout), E = make_case(B, Q, H, seed=Q * 10 + B, tau_mode=tau_mode)
    tab = box_prep(qb, syn.PC_RANGE) if table else None
    out, lse, gq, gt = run_kernels(lin, qb, gout, H, E, tab, wide)
    ref = reference_with_scales(lin[..., :3 * E], lin[..., 3 * E:3 * E + H], qb, H, syn.PC_RANGE, gout)
    name = f"B{B} Q{Q} H{H}{' table' if table else ''} {tau_mode}"
    got = split_grads(gq, gt, E)
    got["lse"] = lse
    for kind, (r, A) in ref.items():
        check(name, kind, got[kind], r, A)
    if Q in (17, 1100):   # negative control: against a reference with one key dropped, every kind must fail
        wrong = reference_with_scales(lin[..., :3 * E], lin[..., 3 * E:3 * E + H], qb, H, syn.PC_RANGE, gout, drop_key=Q // 2)
        for kind, (r, A) in wrong.items():
            _, bad = _bad(kind, got[kind], r, ref[kind][1])
            assert bool(bad.any()), f"{name}: {kind} does not see a dropped key"


@pytest.mark.parametrize("Q", [37, 900, 1100])
def test_forward_ex_bit_identical_and_backward_reproducible(Q):
    (lin, qb, gout), E = make_case(2, Q, 8, seed=Q)
    qkv, tau = lin[..., :3 * E], lin[..., 3 * E:]
    plain = sasa_fused(qkv, tau, qb, 8, syn.PC_RANGE)
    # rac_sasa_fwd_ex with a null lse, through the C-ABI directly
    out_null = torch.empty_like(plain)
    pc = (ctypes.c_float * 6)(*syn.PC_RANGE)
    rc = _lib.lib().rac_sasa_fwd_ex(_lib.ptr(qkv), _lib.ptr(tau), _lib.ptr(qb), None, _lib.ptr(out_null), None, lin.stride(1),
                                    lin.stride(1), 2, Q, 8, 32, pc, _lib.stream_ptr())
    _lib.check(rc, "rac_sasa_fwd_ex")
    r1 = run_kernels(lin, qb, gout, 8, E)
    r2 = run_kernels(lin, qb, gout, 8, E)
    assert torch.equal(plain, out_null) and torch.equal(plain, r1[0])
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)


def _module(E, H, sd=None):
    m = T.ScaleAdaptiveSelfAttention(embed_dims=E, num_heads=H, pc_range=syn.PC_RANGE).eval()
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def test_module_gradients_match_the_reference(golden_dir):
    """fails before rac_sasa_bwd existed: the fused path returned a tensor without history (in_proj / gen_tau grads None)"""
    g = np.load(os.path.join(golden_dir, "sasa_grad_small.npz"))
    m = _module(128, 4, {k: t(g["w:" + k]) for k in KEYS})
    qb = t(g["query_bbox"]).to(DEV).requires_grad_()
    qf = t(g["query_feat"]).to(DEV).requires_grad_()
    out = m(qb, qf, None)
    with torch.no_grad():
        ref_out = m(qb, qf, None)
    assert torch.equal(out.detach(), ref_out)              # grad-mode forward = no_grad forward, bit for bit
    (out * t(g["gout"]).to(DEV)).sum().backward()
    errs = {"out": out, "query_feat": qf.grad, **{k: p.grad for k, p in m.named_parameters()}}
    worst = {}
    for k, v in errs.items():
        assert v is not None, f"{k}: no gradient"
        want = t(g["out" if k == "out" else "g:" + k]).double()
        worst[k] = ((v.detach().cpu().double() - want).abs().max() / want.abs().max()).item()
    print("\nmodule vs reference golden, max |err| / max |value|:", {k: f"{v:.2e}" for k, v in worst.items()})
    # float32 kernels and GEMMs against the reference's float32 CPU autograd (the float64 fakes of test_sasa_grad_cpu.py
    # land within 2.2e-6 of it)
    assert max(worst.values()) < 2e-5, worst
    assert qb.grad is None


def test_f8_module_gradients_against_float64_unfused():
    B, Q, E, H = 1, 900, 256, 8
    torch.manual_seed(3)
    m = _module(E, H)
    with torch.no_grad():
        m.gen_tau.weight.normal_(0, 0.05)
        m.gen_tau.bias.uniform_(0, 2)
    m64 = _module(E, H, {k: v.double() for k, v in m.state_dict().items()}).double()
    g = torch.Generator().manual_seed(4)
    qb = torch.rand(B, Q, 10, generator=g).to(DEV)
    qf = torch.randn(B, Q, E, generator=g).to(DEV)
    gout = torch.randn(B, Q, E, generator=g).to(DEV)
    x = qf.clone().requires_grad_()
    (m(qb, x, None) * gout).sum().backward()
    x64 = qf.double().requires_grad_()
    (m64.forward_unfused(qb.double(), x64, None) * gout.double()).sum().backward()
    p64 = dict(m64.named_parameters())
    pairs = [("query_feat", x.grad, x64.grad)] + [(k, p.grad, p64[k].grad) for k, p in m.named_parameters()]
    worst = {}
    for k, got, want in pairs:
        assert got is not None, k
        worst[k] = ((got.double() - want).abs().max() / want.abs().max()).item()
    print("\nf8 module vs float64 forward_unfused autograd, max |err| / max |value|:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) < 2e-5, worst
