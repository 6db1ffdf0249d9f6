"""The restatement of the refinement tail (tests/refine_ref.py) pinned without a GPU: its float32 forward against its float64
forward, and the closed-form backward -- what rac_refine_bwd implements -- against float64 autograd of the restated forward, with
rows placed ON the gates (proposal[1] / proposal[2] exactly 0 and 1, inside (0, eps), outside [0,1]; boxes whose xy leaves [0,1]
on each side; T = 1; a time_diff_safe of 1.0)."""
import pytest
import torch

import refine_ref as RR

NUM_RAY = 150.0
CASES = [(31, 2, 37, 3, 1), (32, 2, 37, 1, None), (33, 1, 300, 3, 0)]      # seed, B, Q, T, batch with time_diff_safe[:, 1] == 1.0


def check_margins(prop, delta):
    """no row within reach of a gate it is not exactly on, so that float32 and float64 cannot disagree about a gate"""
    inp, computed = RR.gate_margins(prop, delta, NUM_RAY)
    assert inp > RR.INPUT_MARGIN, inp
    assert computed > RR.COMPUTED_MARGIN, computed


@pytest.mark.parametrize("seed,B,Q,T,one_at", CASES)
def test_rows_sit_on_the_gates_or_clear_of_them(seed, B, Q, T, one_at):
    prop, delta, td, _, _ = RR.make_case(seed, B, Q, T, one_at)
    check_margins(prop, delta)
    x = prop[..., 1:3]
    assert (x == 0).any() and (x == 1).any() and ((x > 0) & (x < RR.EPS)).any() and ((x < 1) & (1 - x < RR.EPS)).any()
    assert (x < 0).any() and (x > 1).any()
    ux, uy, _, _ = RR._pre_clamp_xy(prop, delta, NUM_RAY)
    assert (ux > 1).any() and (ux < 0).any() and (uy > 1).any() and (uy < 0).any()
    if one_at is not None and T > 1:
        assert float(td[one_at, 1]) == 1.0


@pytest.mark.parametrize("seed,B,Q,T,one_at", CASES)
def test_float32_forward_equals_float64_to_rounding(seed, B, Q, T, one_at):
    """every output is a chain of fewer than ten float32 operations on values of magnitude <= 12 (the logit at eps), the angle
    of at most 2 pi * 1.01: 16 roundings of max(1, |value|) bound it"""
    prop, delta, td, _, _ = RR.make_case(seed, B, Q, T, one_at)
    got = RR.forward(prop, delta, td, NUM_RAY)
    want = RR.forward(prop.double(), delta.double(), td.double(), NUM_RAY)
    for g, w in zip(got, want):
        assert g.dtype == torch.float32
        assert bool(((g.double() - w).abs() <= 16 * RR.UNIT * w.abs().clamp(min=1)).all())
    if T == 1:
        assert torch.equal(got[0][..., 8:], delta[..., 8:])


@pytest.mark.parametrize("seed,B,Q,T,one_at", CASES)
@pytest.mark.parametrize("which", ["both", "xy", "pred"])
def test_closed_form_is_float64_autograd(seed, B, Q, T, one_at, which):
    prop, delta, td, gp, gx = RR.make_case(seed, B, Q, T, one_at)
    gp, gx = (gp if which != "xy" else None), (gx if which != "pred" else None)
    p, d = prop.double().requires_grad_(), delta.double().requires_grad_()
    pred, xy = RR.forward(p, d, td.double(), NUM_RAY)
    loss = sum((o * g.double()).sum() for o, g in ((pred, gp), (xy, gx)) if g is not None)
    loss.backward()
    gd, gpr = RR.closed_form_bwd(prop, delta, td, NUM_RAY, gp, gx)
    md, mpr = RR.closed_form_bwd(prop, delta, td, NUM_RAY, gp, gx, magnitude=True)
    for got, want, mag in ((gd, d.grad, md), (gpr, p.grad, mpr)):
        assert bool(((got - want).abs() <= 1e-13 * mag + 1e-300).all())
        assert bool((mag >= got.abs() * (1 - 1e-12)).all())
    assert bool((gpr[..., 3:] == 0).all())
    # the gates did something: a blocked proposal gradient beside a passed one, a blocked xy beside a passed one
    assert bool((gpr[..., 1] == 0).any()) and bool((gpr[..., 1] != 0).any())


def test_absent_gradient_is_a_zero_gradient():
    prop, delta, td, gp, gx = RR.make_case(34, 2, 37, 3, 1)
    a = RR.closed_form_bwd(prop, delta, td, NUM_RAY, None, gx)
    b = RR.closed_form_bwd(prop, delta, td, NUM_RAY, torch.zeros_like(gp), gx)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_restatement_is_the_packages_torch_formulation():
    """the same ops as the package's own torch helpers (the comparator plan of the parity tests)"""
    from racformer_amd.bbox_utils import inverse_sigmoid, theta_d2xy_coods
    prop, delta, td, _, _ = RR.make_case(35, 2, 37, 3, None)
    assert torch.equal(inverse_sigmoid(prop[..., 1:3]), RR.inverse_sigmoid(prop[..., 1:3]))
    pred, xy = RR.forward(prop, delta, td, NUM_RAY)
    assert torch.equal(theta_d2xy_coods(pred), xy)
