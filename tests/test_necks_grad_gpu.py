"""The image necks' backward on the MI355X (racformer_amd/necks.py ``fused_grad``; csrc/fpn_lateral_bwd.hip, the data-gradient
instantiation of csrc/fpn_lateral.hip): one call of each new kernel against float64, then both modules under autograd.

Reference: float64 CPU autograd through tests/necks_ref.py (``lateral``, ``fpn``, ``custom_fpn``) on seeded inputs.

Kernel level.  Metric: worst |err| / A in units of 2^-24, A the same sum with every term taken in absolute value.  Criterion, the one
of tests/test_temporal_fusion_grad_gpu.py: kernel <= max(2 x the figure of torch's CPU float32 autograd on the same inputs, 8) -- the
factor of two is the allowance for another summation order, the floor the split's own bound (each operand rounded at 2^-23, the
dropped lo*lo term 2^-22: 2^-21 of A in all).  The merge is exact float addition in a fixed order and is compared BITWISE with an
fp32 index_add that adds each coarse pixel's children in the same (row-major) order.

  case    images  Cin   H x W     why
  c32     3       32    8 x 22    one K chunk of the forward, a 64-channel ci tile with half of it past Cin, 176 pixels = 5.5 K units
  c96     3       96    8 x 22    odd chunk count, ci tile of 64 twice with a ragged second
  c256    3       256   8 x 22    the common case: 128-channel ci tiles, one block of 256 data-gradient channels
  c2048   3       2048  8 x 22    the deepest level: 8 blocks of data-gradient channels, 16 ci tiles
  odd     2       96    7 x 11    77 pixels: 4-byte loads, ragged last unit
  odd2048 2       2048  7 x 11    the same on the widest level
  one     1       32    1 x 1     a single pixel
  big     6       32    64 x 176  the 128-pixel tile of the data gradient, 423 K ranges of the weight gradient

Module level (necks_ref.LSS and necks_ref.FPN4, a random output gradient per level): every input and parameter gradient within
max(2 x the torch route's own error against float64 on the device, 1e-5) of its largest element; the forward under ``fused_grad``
bitwise the no-grad route's; two backward runs bitwise equal; frozen parameters / detached inputs / a detached stage-0 input leave the
remaining gradients bitwise unchanged and skip the launches nobody asked for.

Measured on an MI355X, kernel | torch's CPU float32 autograd (units of 2^-24):
            c32         c96         c256        c2048       odd         odd2048     one         big
  dX        2.61|3.23   2.16|4.27   2.71|4.90   3.87|5.53   2.15|3.60   4.00|6.88   1.55|2.06   3.11|2.99
  dW        0.70|1.27   0.82|1.87   0.87|2.00   1.12|2.07   1.07|2.26   1.29|3.29   6.46|0.99   0.32|0.25
  db        0.34|1.61   0.44|1.46   0.25|2.07   0.34|1.76   0.81|2.16   0.39|1.61   0.00|0.00   0.11|1.71
  ("one" is a single product: dW sits at the split's own bound, the floor of 8, with nothing to average over.)
  c256 with G x 1e-6: dW 0.98, db 0.31, dX 2.68; x 1e4: 1.02, 0.51, 2.65.  One pixel x 1e3: the other pixels' dX 2.71|4.90.
  The merge against float64: at most 2.2 units (the fp32 additions themselves).
  Modules, of the largest element, HIP | torch route: inputs <= 7.9e-7|8.3e-7, 3x3 weights <= 2.7e-7|4.8e-7, lateral weights
  <= 1.2e-6|7.2e-7, lateral biases <= 2.1e-6|5.4e-7, 3x3 biases equal (both are torch sums).

Every (kernel, torch32) pair is printed before it is asserted; RAC_NECKS_GRAD_ERRORS=<file> writes them as JSON
(tools/necks_bench.py --errors copies them into the record)."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import necks_ref as NR
from racformer_amd import necks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNIT = 2.0 ** -24
CASES = {"c32": (3, 32, 8, 22), "c96": (3, 96, 8, 22), "c256": (3, 256, 8, 22), "c2048": (3, 2048, 8, 22), "odd": (2, 96, 7, 11),
         "odd2048": (2, 2048, 7, 11), "one": (1, 32, 1, 1), "big": (6, 32, 64, 176)}
PAIRS = []
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _error_pairs():
    yield
    path = os.environ.get("RAC_NECKS_GRAD_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump(PAIRS, f, indent=1)


def _inputs(case):
    n, cin, h, w = CASES[case]
    seed = 5000 + 17 * sorted(CASES).index(case)
    x = torch.from_numpy(NR.syn.rng_normal(seed, (n, cin, h, w)))
    wt = torch.from_numpy(NR.syn.rng_normal(seed + 1, (256, cin, 1, 1), 1.0 / float(np.sqrt(cin))))
    b = torch.from_numpy(NR.syn.rng_normal(seed + 2, (256,), 0.1))
    g = torch.from_numpy(NR.syn.rng_normal(seed + 3, (n, 256, h, w)))
    return x, wt, b, g


def _autograd64(x, wt, b, g):
    """(dX, dW, db) by float64 autograd through necks_ref.lateral"""
    x, wt, b = (t.double().clone().requires_grad_() for t in (x, wt, b))
    NR.lateral(x, wt, b).backward(g.double())
    return x.grad, wt.grad, b.grad


def _autograd32(x, wt, b, g):
    x, wt, b = (t.float().clone().requires_grad_() for t in (x, wt, b))
    F.conv2d(x, wt, b).backward(g.float())
    return x.grad, wt.grad, b.grad


def metric(got, want, mag, scale=1.0):
    """worst |err| / A in units of 2^-24 (``scale``: the factor the gradient was multiplied by)"""
    err = (got.detach().double().cpu() - want * scale).abs()
    return float((err / (mag * abs(scale)).clamp_min(1e-300)).max()) / UNIT


def reference(case):
    """float64 gradients, their magnitudes A and torch's CPU float32 figures -- computed once per case, never modified"""
    if case not in _REF:
        x, wt, b, g = _inputs(case)
        want = _autograd64(x, wt, b, g)
        mag = _autograd64(x.abs(), wt.abs(), b.abs(), g.abs())
        t32 = [metric(a, r, m) for a, r, m in zip(_autograd32(x, wt, b, g), want, mag)]
        _REF[case] = dict(want=want, mag=mag, torch32=t32)
    return _REF[case]


def judge(what, fig, t32):
    print(f"\n{what}: kernel {fig:.3f} | torch32 {t32:.3f}")
    PAIRS.append(dict(case=what, kernel=fig, torch32=t32))
    assert fig <= max(2.0 * t32, 8.0), f"{what}: {fig:.3f} units against torch float32 {t32:.3f}"


def run_dgrad(wt, g):
    packed = necks.pack_lateral_weight_t(wt.to(DEV))
    out = necks.fpn_lateral_dgrad(g.to(DEV).contiguous(), packed, int(wt.shape[1]))
    torch.cuda.synchronize()
    return out.cpu()


def run_wgrad(g, x, bias=True):
    dw, db = necks.fpn_lateral_wgrad(g.to(DEV).contiguous(), x.to(DEV).contiguous(), bias=bias)
    torch.cuda.synchronize()
    return dw.cpu(), (db.cpu() if db is not None else None)


# ------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("case", list(CASES))
def test_lateral_dgrad_against_float64(case):
    x, wt, b, g = _inputs(case)
    ref = reference(case)
    got = run_dgrad(wt, g)
    assert got.shape == x.shape and got.is_contiguous() and bool(torch.isfinite(got).all())
    judge(f"dgrad {case}", metric(got, ref["want"][0], ref["mag"][0]), ref["torch32"][0])


@pytest.mark.parametrize("case", list(CASES))
def test_lateral_wgrad_against_float64(case):
    x, wt, b, g = _inputs(case)
    ref = reference(case)
    dw, db = run_wgrad(g, x)
    assert dw.shape == wt.shape and db.shape == b.shape and bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
    judge(f"wgrad {case} dW", metric(dw, ref["want"][1], ref["mag"][1]), ref["torch32"][1])
    judge(f"wgrad {case} db", metric(db, ref["want"][2], ref["mag"][2]), ref["torch32"][2])
    dw2, none = run_wgrad(g, x, bias=False)
    assert none is None and torch.equal(dw2, dw)


def test_the_big_case_takes_the_wide_tile_and_several_k_ranges():
    n, cin, h, w = CASES["big"]
    assert n * ((h * w + 127) // 128) >= 256 and necks.lateral_wgrad_k_splits(n, h, w, cin) > 100
    assert necks.lateral_wgrad_k_splits(*[CASES["c256"][i] for i in (0, 2, 3, 1)]) > 1


@pytest.mark.parametrize("scale", [1e-6, 1e4])
def test_wgrad_scale_of_the_gradient(scale):
    """the operands take their power-of-two scales from their own maxima, per channel and K range"""
    x, wt, b, g = _inputs("c256")
    ref = reference("c256")
    dw, db = run_wgrad(g * scale, x)
    judge(f"wgrad c256 G x {scale:g} dW", metric(dw, ref["want"][1], ref["mag"][1], scale), ref["torch32"][1])
    judge(f"wgrad c256 G x {scale:g} db", metric(db, ref["want"][2], ref["mag"][2], scale), ref["torch32"][2])
    judge(f"dgrad c256 G x {scale:g}", metric(run_dgrad(wt, g * scale), ref["want"][0], ref["mag"][0], scale), ref["torch32"][0])


def test_zero_gradient_gives_exact_zeros():
    x, wt, b, g = _inputs("c96")
    z = torch.zeros_like(g)
    dw, db = run_wgrad(z, x)
    dx = run_dgrad(wt, z)
    for name, t in (("dW", dw), ("db", db), ("dX", dx)):
        assert bool((t == 0).all()) and not bool(torch.isnan(t).any()), name


def test_dgrad_one_large_pixel_leaves_the_others_alone():
    """One pixel of G at 1e3 times the rest: the scale of G is per pixel, so the other pixels' dX keep their accuracy (A is a sum
    over channels of ONE pixel, so the metric judges every pixel against its own magnitude)."""
    x, wt, b, g = _inputs("c256")
    g = g.clone()
    g[1, :, 3, 5] *= 1.0e3
    want, mag = _autograd64(x, wt, b, g)[0], _autograd64(x.abs(), wt.abs(), b.abs(), g.abs())[0]
    t32 = _autograd32(x, wt, b, g)[0]
    got = run_dgrad(wt, g)
    keep = torch.ones(g.shape[0], 1, *g.shape[2:], dtype=torch.bool)
    keep[1, :, 3, 5] = False
    keep = keep.expand_as(want)
    judge("dgrad one pixel x1e3, whole map", metric(got, want, mag), metric(t32, want, mag))
    judge("dgrad one pixel x1e3, the other pixels", metric(got[keep], want[keep], mag[keep]), metric(t32[keep], want[keep], mag[keep]))


MERGES = [((4, 6), (7, 11), 2, 256), ((4, 11), (8, 22), 3, 256), ((1, 1), (1, 1), 1, 256), ((7, 11), (7, 11), 2, 256),
          ((1, 1), (7, 11), 2, 256), ((3, 5), (7, 11), 2, 40), ((32, 88), (64, 176), 6, 256)]


@pytest.mark.parametrize("hw,fine,n,c", MERGES)
def test_merge_is_an_ordered_index_add_bitwise(hw, fine, n, c):
    """A ragged top, an exact half, single pixels, a top as large as the level, everything into one pixel, a ratio above two with
    another channel count, and the f8 ratio on maps of several workgroups -- with and without ``a``."""
    a = torch.from_numpy(NR.syn.rng_normal(900 + hw[0], (n, c) + hw))
    gf = torch.from_numpy(NR.syn.rng_normal(901 + fine[0], (n, c) + fine))
    sh = torch.tensor([necks.nearest_src(d, hw[0], fine[0]) for d in range(fine[0])])
    sw = torch.tensor([necks.nearest_src(d, hw[1], fine[1]) for d in range(fine[1])])
    idx = (sh[:, None] * hw[1] + sw[None, :]).reshape(-1)                      # coarse pixel of every fine pixel, row-major
    for first in (a, None):
        want = (first.clone() if first is not None else torch.zeros_like(a)).reshape(n * c, -1)
        want.index_add_(1, idx, gf.reshape(n * c, -1))                         # ascending fine index = row-major per coarse pixel
        got = necks.fpn_merge_backward(first.to(DEV) if first is not None else None, gf.to(DEV), size=hw)
        torch.cuda.synchronize()
        assert got.shape == (n, c) + hw and torch.equal(got.cpu().reshape(n * c, -1), want)
    # and it is the gradient of the forward's top-down term: float64 autograd through necks_ref.lateral's ``top``
    if c == 256 and hw[0] * hw[1] <= 100:
        top = torch.zeros((n, 256) + hw, dtype=torch.double, requires_grad=True)
        NR.lateral(torch.zeros((n, 32) + fine), torch.zeros(256, 32, 1, 1), None, top).backward(gf.double())
        top_mag = torch.zeros((n, 256) + hw, dtype=torch.double, requires_grad=True)
        NR.lateral(torch.zeros((n, 32) + fine), torch.zeros(256, 32, 1, 1), None, top_mag).backward(gf.double().abs())
        only = necks.fpn_merge_backward(None, gf.to(DEV), size=hw).cpu()
        fig = metric(only, top.grad, top_mag.grad)
        print(f"\nmerge {hw} <- {fine}: {fig:.3f} units against float64")
        assert fig <= 8.0
    only_a = necks.fpn_merge_backward(a.to(DEV), None)
    assert torch.equal(only_a.cpu(), a)


# ------------------------------------------------------------------------------------------------------------------ modules
def shapes_of(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def _module(kind):
    if kind == "lss":
        m = necks.CustomFPN(NR.LSS["channels"], 256, num_outs=1, start_level=0, out_ids=[0])
        spec, levels = NR.LSS, [0]
    else:
        m = necks.FPN(NR.FPN4["channels"], 256, 4)
        spec, levels = NR.FPN4, [0, 1, 2, 3]
    sd = NR.fill_state(shapes_of(m), 4100 + len(levels))
    m.load_state_dict(sd)
    xs = NR.make_inputs(4200 + len(levels), spec["images"], spec["channels"], spec["maps"], relu=True)
    gouts = [torch.from_numpy(NR.syn.rng_normal(4300 + i, (spec["images"], 256) + spec["maps"][i])) for i in levels]
    return m, sd, xs, gouts


def _float64(kind, sd, xs, gouts):
    sd = {k: v.double().clone().requires_grad_() for k, v in sd.items()}
    xs = [x.double().clone().requires_grad_() for x in xs]
    out = NR.custom_fpn(sd, xs) if kind == "lss" else NR.fpn(sd, xs)
    outs = (out,) if kind == "lss" else out
    torch.autograd.backward(outs, [g.double() for g in gouts])
    return {**{f"input{i}": x.grad for i, x in enumerate(xs)}, **{k: v.grad for k, v in sd.items()}}


def _run(kind, base, xs, gouts, switch, req_inputs=None, req_params=True):
    m = copy.deepcopy(base).to(DEV)
    m.fused_grad = switch
    for p in m.parameters():
        p.requires_grad_(req_params)
    req_inputs = [True] * len(xs) if req_inputs is None else req_inputs
    xd = [x.to(DEV).requires_grad_(r) for x, r in zip(xs, req_inputs)]
    assert m.hip_grad_route(xd) == bool(switch) and not m.hip_route(xd)
    out = m(xd)
    outs = (out,) if kind == "lss" else out
    torch.autograd.backward(outs, [g.to(DEV) for g in gouts])
    torch.cuda.synchronize()
    grads = {**{f"input{i}": x.grad for i, x in enumerate(xd)}, **{k: p.grad for k, p in m.named_parameters()}}
    return [o.detach() for o in outs], grads


@pytest.fixture(scope="module", params=["lss", "fpn4"])
def neck(request):
    kind = request.param
    m, sd, xs, gouts = _module(kind)
    outs, grads = _run(kind, m, xs, gouts, True)
    return dict(kind=kind, m=m, sd=sd, xs=xs, gouts=gouts, outs=outs, grads=grads)


def test_module_gradients_against_float64(neck):
    kind = neck["kind"]
    g64 = _float64(kind, neck["sd"], neck["xs"], neck["gouts"])
    _, g_off = _run(kind, neck["m"], neck["xs"], neck["gouts"], False)
    g_on = neck["grads"]
    assert set(g_on) == set(g64) == set(g_off)
    for name, want in g64.items():
        big = float(want.abs().max())
        e_on = float((g_on[name].double().cpu() - want).abs().max()) / big
        e_off = float((g_off[name].double().cpu() - want).abs().max()) / big
        print(f"\n{kind} {name}: on {e_on:.3e}  off {e_off:.3e}")
        PAIRS.append(dict(case=f"module {kind} {name}", on=e_on, off=e_off))
        assert g_on[name].shape == want.shape
        assert e_on <= max(2.0 * e_off, 1e-5), f"{kind} {name}: {e_on:.3e} against the torch route's {e_off:.3e}"


def test_forward_under_fused_grad_is_the_no_grad_route_bitwise(neck):
    m = copy.deepcopy(neck["m"]).to(DEV)
    xd = [x.to(DEV) for x in neck["xs"]]
    with torch.no_grad():
        assert m.hip_route(xd)
        out = m(xd)
    plain = (out,) if neck["kind"] == "lss" else out
    assert len(plain) == len(neck["outs"])
    for a, b in zip(plain, neck["outs"]):
        assert torch.equal(a, b)


def test_two_backward_runs_give_the_same_bits(neck):
    _, again = _run(neck["kind"], neck["m"], neck["xs"], neck["gouts"], True)
    for name, g in neck["grads"].items():
        assert torch.equal(g, again[name]), name


def _count(monkeypatch, name):
    calls, real = [], getattr(necks, name)
    monkeypatch.setattr(necks, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


def test_frozen_parameters_leave_the_input_gradients_bitwise(neck, monkeypatch):
    wg, cw = _count(monkeypatch, "fpn_lateral_wgrad"), _count(monkeypatch, "conv3x3_wgrad")
    _, grads = _run(neck["kind"], neck["m"], neck["xs"], neck["gouts"], True, req_params=False)
    assert not wg and not cw
    for name, g in grads.items():
        if name.startswith("input"):
            assert torch.equal(g, neck["grads"][name]), name
        else:
            assert g is None, name


def test_detached_inputs_leave_the_parameter_gradients_bitwise(neck, monkeypatch):
    dg = _count(monkeypatch, "fpn_lateral_dgrad")
    _, grads = _run(neck["kind"], neck["m"], neck["xs"], neck["gouts"], True, req_inputs=[False] * len(neck["xs"]))
    assert not dg
    for name, g in grads.items():
        if name.startswith("input"):
            assert g is None, name
        else:
            assert torch.equal(g, neck["grads"][name]), name


def test_detached_stage0_input_skips_its_data_gradient_only(neck, monkeypatch):
    dg = _count(monkeypatch, "fpn_lateral_dgrad")
    levels = len(neck["xs"])
    _, grads = _run(neck["kind"], neck["m"], neck["xs"], neck["gouts"], True, req_inputs=[False] + [True] * (levels - 1))
    assert len(dg) == levels - 1
    assert grads["input0"] is None
    for name, g in grads.items():
        if name != "input0":
            assert torch.equal(g, neck["grads"][name]), name


def test_without_the_switch_training_takes_the_torch_route(neck, monkeypatch):
    merges, wgrads = _count(monkeypatch, "fpn_merge_backward"), _count(monkeypatch, "fpn_lateral_wgrad")
    _run(neck["kind"], neck["m"], neck["xs"], neck["gouts"], False)
    assert not merges and not wgrads
