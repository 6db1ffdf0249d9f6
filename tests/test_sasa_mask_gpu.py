"""The masked SASA kernels on the MI355X: rac_sasa_fwd_mask (register-resident up to Q = 1024, streaming above) and
rac_sasa_bwd_mask (the two-role backward with the mask in both roles).

  * every kind (dq, dk, dv, dtau, lse) element by element against float64 (tests/sasa_mask_ref.py) under the bound of
    tests/test_sasa_grad_gpu.py, ``|got - ref| <= 64 * 2**-24 * A + 1e-30``, over the sizes around a tile, a mask word and the
    switch between the two forward kernels, four kinds of mask (the denoising layout, random, whole tiles blocked, garbage in
    the padding bits), both box_table modes, the strided 776-wide lin; gradient buffers pre-filled with NaN;
  * a negative control: against the reference with ONE blocked bit cleared every kind falls outside the bound;
  * with an all-zero mask both kernels are bit-identical to the unmasked ones; the masked backward is bit-reproducible;
  * tile skipping changes no bit: a run in which every skipped tile is made non-skippable (one bit cleared per tile, on rows
    that carry a zero output gradient) gives the same bits everywhere outside those rows;
  * the module against the reference's own autograd under the mask (tests/golden/sasa_mask_grad_small.npz)."""
import os

import numpy as np
import pytest
import torch

import sasa_mask_ref as MR
from racformer_amd import synthetic as syn
from racformer_amd import transformer as T
from racformer_amd.fused import box_prep, pack_attn_mask, sasa_backward, sasa_fused
from test_sasa_grad_gpu import DEV, KEYS, TINY, U, make_case, split_grads, t

pytestmark = pytest.mark.gpu
# the bound of tests/test_sasa_grad_gpu.py, one factor for every kind; ``out`` (a sum of at most Q products P v, like dv) with it
K = {"dq": 64.0, "dk": 64.0, "dv": 64.0, "dtau": 64.0, "lse": 64.0, "out": 64.0}
WORST = {}


def _bad(kind, got, ref, A):
    err = (got.double() - ref).abs()
    return err, ~(err <= K[kind] * U * A + TINY)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nmasked kernels, worst err/A per kind, in units of 2**-24 (bound K = 64):")
    for name in sorted(WORST):
        print(f"  {name:>52s}: {WORST[name] / U:9.3f}")


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


def run_kernels(lin, qb, gout, H, E, mask, table=None, wide_grad=True):
    qkv, tau = lin[..., :3 * E], lin[..., 3 * E:3 * E + H]
    B, Q, _ = qb.shape
    lse = torch.full((B, H, Q), float("nan"), device=DEV)
    out = sasa_fused(qkv, tau, qb, H, syn.PC_RANGE, box_table=table, lse_out=lse, mask=mask)
    if wide_grad:   # one buffer shaped like lin, pre-filled with NaN: every element of the two slices must be written
        buf = torch.full(lin.shape, float("nan"), device=DEV)
        gq, gt = buf[..., :3 * E], buf[..., 3 * E:3 * E + H]
    else:
        gq = torch.full((B, Q, 3 * E), float("nan"), device=DEV)
        gt = torch.full((B, Q, H), float("nan"), device=DEV)
    sasa_backward(qkv, tau, qb, H, syn.PC_RANGE, out, lse, gout, box_table=table, grad_qkv=gq, grad_tau=gt, mask=mask)
    torch.cuda.synchronize()
    return out, lse, gq, gt


# (B, Q, heads, (groups, single) of the denoising layout)
SHAPES = [(4, 1, 4, (0, 0)), (2, 15, 4, (3, 2)), (2, 16, 4, (3, 3)), (2, 17, 4, (3, 3)), (2, 33, 4, (3, 5)), (2, 41, 4, (3, 7)),
          (2, 64, 8, (3, 10)), (1, 1024, 2, (10, 30)), (1, 1040, 2, (10, 14)), (1, 1300, 2, (10, 40))]
MASKS = ["dn", "random", "tiles", "garbage"]


def make_mask(kind, Q, dn):
    """-> (bool mask on the CPU, PackedAttnMask on the GPU)"""
    if kind == "dn":
        m = MR.dn_layout(Q, *dn)
        return m, pack_attn_mask(m.to(DEV))                              # through the product's packer
    if kind == "random":
        m = MR.random_mask(Q, seed=Q)
        return m, pack_attn_mask(m.to(DEV))
    if kind == "tiles":
        m = MR.tile_mask(Q, seed=Q + 1)
        return m, MR.packed(m, DEV, extra_words=1)                       # a row stride wider than ceil(Q/32)
    m = MR.dn_layout(Q, *dn) | MR.tile_mask(Q, seed=Q + 2, tile_density=0.2)
    return m, MR.packed(m, DEV, extra_words=1, garbage_seed=Q)           # ones past Q: ignored


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("B,Q,H,dn", SHAPES)
def test_masked_kernel_gradients_against_float64(B, Q, H, dn, kind):
    (lin, qb, gout), E = make_case(B, Q, H, seed=Q * 10 + B)
    # both box_table modes and both gradient destinations over the (shape, mask) grid
    n = SHAPES.index((B, Q, H, dn)) + MASKS.index(kind)
    table, wide = bool(n & 1), bool(n & 2) or H == 8       # (H = 8: the strided 776-wide lin and its one gradient buffer)
    mask, pk = make_mask(kind, Q, dn)
    assert not bool(mask.all(dim=1).any()), "a row without an allowed key is outside the contract"
    tab = box_prep(qb, syn.PC_RANGE) if table else None
    out, lse, gq, gt = run_kernels(lin, qb, gout, H, E, pk, tab, wide)
    qkv, tau = lin[..., :3 * E], lin[..., 3 * E:3 * E + H]
    ref = MR.reference_with_scales(qkv, tau, qb, H, syn.PC_RANGE, gout, mask)
    name = f"B{B} Q{Q} H{H} {kind}{' table' if table else ''}"
    got = split_grads(gq, gt, E)
    got["lse"] = lse
    got["out"] = out
    for k_, (r, A) in ref.items():
        check(name, k_, got[k_], r, A)
    # negative control: against the reference with ONE blocked bit cleared -- where the freed probability is largest in
    # (batch 0, head 0), confirmed in float64 not to be negligible -- every kind must fall outside the bound
    if kind == "dn" and dn[0] and Q in (41, 1040) and dn[0] * dn[1] < Q:
        wrong_mask = mask.clone()
        p = MR.freed_probability(qkv, tau, qb, H, syn.PC_RANGE, mask)
        flat = int(p.argmax())
        i, j = flat // Q, flat % Q
        assert float(p[i, j]) > 1e-3, f"the freed probability {float(p[i, j]):.3e} is negligible: the control would show nothing"
        wrong_mask[i, j] = False
        wrong = MR.reference_with_scales(qkv, tau, qb, H, syn.PC_RANGE, gout, wrong_mask)
        for k_, (r, _) in wrong.items():
            _, bad = _bad(k_, got[k_], r, ref[k_][1])
            assert bool(bad.any()), f"{name}: {k_} does not see the cleared bit ({i}, {j})"


@pytest.mark.parametrize("Q", [37, 900])
def test_all_zero_mask_is_bit_identical_to_the_unmasked_kernels(Q):
    (lin, qb, gout), E = make_case(2, Q, 8, seed=Q)
    qkv, tau = lin[..., :3 * E], lin[..., 3 * E:]
    zero = pack_attn_mask(torch.zeros(Q, Q, dtype=torch.bool, device=DEV))
    lse0 = torch.empty(2, 8, Q, device=DEV)
    out0 = sasa_fused(qkv, tau, qb, 8, syn.PC_RANGE, lse_out=lse0)
    gq0, gt0 = sasa_backward(qkv, tau, qb, 8, syn.PC_RANGE, out0, lse0, gout)
    out1, lse1, gq1, gt1 = run_kernels(lin, qb, gout, 8, E, zero)
    out_nolse = sasa_fused(qkv, tau, qb, 8, syn.PC_RANGE, mask=zero)          # null lse
    assert torch.equal(out0, out1) and torch.equal(lse0, lse1) and torch.equal(out0, out_nolse)
    assert torch.equal(gq0, gq1) and torch.equal(gt0, gt1)


@pytest.mark.parametrize("Q,dn", [(41, (3, 7)), (1300, (10, 40))])
def test_masked_backward_is_bit_reproducible(Q, dn):
    (lin, qb, gout), E = make_case(1, Q, 4, seed=Q + 5)
    pk = pack_attn_mask(MR.dn_layout(Q, *dn).to(DEV))
    r1 = run_kernels(lin, qb, gout, 4, E, pk)
    r2 = run_kernels(lin, qb, gout, 4, E, pk)
    for a, b in zip(r1, r2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("B,Q,H,dn", [(2, 41, 4, (3, 7)), (2, 64, 8, (3, 10)), (1, 1300, 2, (10, 40))])
def test_tile_skipping_changes_no_bit(B, Q, H, dn):
    """mask M' = M with one bit cleared in every 16 x 16 tile M blocks whole, at the tile's first row and column: no tile of
    M' is skipped where M skips.  The cleared rows (i % 16 == 0) carry a zero output gradient in both runs, so they
    contribute exact zeros to dk and dv whatever their probabilities; every other row is the same row under both masks."""
    (lin, qb, gout), E = make_case(B, Q, H, seed=Q + 9)
    gout[:, ::16] = 0.0
    m = MR.dn_layout(Q, *dn)
    nt = (Q + 15) // 16
    padded = torch.ones(nt * 16, nt * 16, dtype=torch.bool)
    padded[:Q, :Q] = m
    whole = padded.view(nt, 16, nt, 16).permute(0, 2, 1, 3).reshape(nt, nt, 256).all(-1)
    assert int(whole.sum()) > 0, "the layout must have tiles to skip"
    m2 = m.clone()
    for ti, tj in whole.nonzero().tolist():
        m2[ti * 16, tj * 16] = False
    a = run_kernels(lin, qb, gout, H, E, pack_attn_mask(m.to(DEV)))
    b = run_kernels(lin, qb, gout, H, E, pack_attn_mask(m2.to(DEV)))
    keep = torch.ones(Q, dtype=torch.bool, device=DEV)
    keep[::16] = False
    assert torch.equal(a[0][:, keep], b[0][:, keep]), "out"
    assert torch.equal(a[1][:, :, keep], b[1][:, :, keep]), "lse"
    ga, gb = split_grads(a[2], a[3], E), split_grads(b[2], b[3], E)
    assert torch.equal(ga["dq"][:, keep], gb["dq"][:, keep]) and torch.equal(ga["dtau"][:, keep], gb["dtau"][:, keep])
    assert torch.equal(ga["dk"], gb["dk"]) and torch.equal(ga["dv"], gb["dv"])


def test_module_gradients_match_the_reference_under_the_mask(golden_dir):
    """fails on the parent commit: a masked call took forward_unfused (and before that, the fused path ignored no mask at all)"""
    g = np.load(os.path.join(golden_dir, "sasa_mask_grad_small.npz"))
    m = T.ScaleAdaptiveSelfAttention(embed_dims=128, num_heads=4, pc_range=syn.PC_RANGE).eval()
    m.load_state_dict({k: t(g["w:" + k]) for k in KEYS})
    m = m.to(DEV)
    calls = []
    real_fwd, real_bwd = T.sasa_fused, T.sasa_backward
    mask = t(g["attn_mask"]).to(DEV)
    qb = t(g["query_bbox"]).to(DEV).requires_grad_()
    qf = t(g["query_feat"]).to(DEV).requires_grad_()
    try:
        T.sasa_fused = lambda *a, **k: calls.append(("fwd", "mask" in k)) or real_fwd(*a, **k)
        T.sasa_backward = lambda *a, **k: calls.append(("bwd", "mask" in k)) or real_bwd(*a, **k)
        out = m(qb, qf, mask)
        with torch.no_grad():
            ref_out = m(qb, qf, pack_attn_mask(mask))
        (out * t(g["gout"]).to(DEV)).sum().backward()
    finally:
        T.sasa_fused, T.sasa_backward = real_fwd, real_bwd
    assert calls == [("fwd", True), ("fwd", True), ("bwd", True)], "the masked call must take the fused kernels"
    assert torch.equal(out.detach(), ref_out)              # grad-mode forward = no_grad forward, bit for bit
    errs = {"out": out, "query_feat": qf.grad, **{k: p.grad for k, p in m.named_parameters()}}
    worst = {}
    for k, v in errs.items():
        assert v is not None, f"{k}: no gradient"
        want = t(g["out" if k == "out" else "g:" + k]).double()
        worst[k] = ((v.detach().cpu().double() - want).abs().max() / want.abs().max()).item()
    print("\nmasked module vs reference golden, max |err| / max |value|:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) < 2e-5, worst
    assert qb.grad is None
