"""_TemporalFusionCore on the MI355X: the temporal-fusion convolution under autograd with its HIP backward -- the data gradients
on rac_conv3x3_fwd (image of the output gradient, transposed and flipped weights), the weight gradient on rac_conv3x3_wgrad
(transposed LDS reads, K split with a fixed summation order), the bias gradient a sum.

Reference: float64 CPU autograd of F.conv2d on the same inputs.  Metric: worst |err| / A in units of 2^-24, A the same sum with
every term taken in absolute value.  Criterion per gradient: kernel <= max(2 x the figure of torch's CPU float32 autograd on the
same inputs, 8) -- the factor of two is the allowance for another summation order, the floor the split's own bound (each
operand rounded at 2^-23, the dropped lo*lo term 2^-22: 2^-21 of A in all).

  case  N  H x W     hidden  why
  A     1  16 x 16   64      exactly one 256-pixel tile
  B     3  20 x 16   64      full tile + ragged tile, odd frame count for the K split
  C     2  8 x 12    32      one ragged tile, W not a power of two, Cin = 288 (odd chunk count)
  D     2  2 x 128   64      widest supported row, every pixel on a border row
  E     4  32 x 32   64      several K ranges per output tile

Measured on an MI355X, kernel | torch's CPU float32 autograd (units of 2^-24; the test prints them before it asserts):
            A            B            C            D            E
  forward   3.15         3.22         3.22         3.06         4.27         (kernel alone, bound 8)
  grad_x    2.64|0.68    2.55|0.71    2.85|0.73    2.59|0.73    3.80|0.82
  grad_hid  2.85|0.61    2.86|0.73    1.93|0.56    2.22|0.72    3.06|0.70
  grad_w    1.45|5.34    0.96|5.35    1.60|5.48    1.60|5.21    0.56|6.37
  grad_b    0.59|1.60    0.20|1.22    0.47|1.45    0.28|1.80    0.31|1.14
  case A with W[:, 256:] = 0 (grad_hid exactly zero): 2.64|0.68, 1.45|5.34, 0.59|1.60 (x, w, b).
  case A with grad_output x 1e-6: 2.87, 2.27, 1.62, 0.49; x 1e+4: 3.22, 2.16, 1.42, 0.45 (x, hid, w, b).
  The data gradients sit at the split's own level (the floor of 8), above torch's float32: every product carries the two
  operands' 2^-23 roundings, where float32 rounds only its running sum; the weight gradient, a sum over all pixels, is well
  below torch's.

Module level (RadarBEVTemporalEncoder, B = 1, T = 5, 16 x 16): every gradient within max(2 x the library route's own error against
float64, 1e-5) of its largest element; the two routes' outputs within 1e-4 of the largest element.
  Measured: forward on - off 4.4e-6 of 2.39; gradients on | off against float64, of the largest element: input 1.2e-6|6.7e-7,
  temporal_fusion.weight 1.9e-7|3.3e-7, temporal_fusion.bias 1.2e-7|8.6e-8, every other parameter <= 1.3e-6|8.7e-7."""
import copy

import pytest
import torch
import torch.nn.functional as F

from racformer_amd import fused
from racformer_amd import transformer as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNIT = 2.0 ** -24
CASES = {"A": (1, 16, 16, 64), "B": (3, 20, 16, 64), "C": (2, 8, 12, 32), "D": (2, 2, 128, 64), "E": (4, 32, 32, 64)}
NAMES = ("grad_x", "grad_hid", "grad_w", "grad_b")
_REF = {}


def _inputs(case):
    N, H, W, hd = CASES[case]
    g = torch.Generator().manual_seed(1000 + ord(case))
    x = torch.randn(N, 256, H, W, generator=g)
    hid = torch.randn(N, hd, H, W, generator=g) * 0.5
    w = torch.randn(256, 256 + hd, 3, 3, generator=g) * 0.03
    b = torch.randn(256, generator=g) * 0.1
    gy = torch.randn(N, 256, H, W, generator=g)
    return x, hid, w, b, gy


def _autograd(x, hid, w, b, gy, dtype):
    x, hid, w, b = (t.to(dtype).clone().requires_grad_() for t in (x, hid, w, b))
    out = F.conv2d(torch.cat([x, hid], dim=1), w, b, padding=1)
    out.backward(gy.to(dtype))
    return out.detach(), (x.grad, hid.grad, w.grad, b.grad)


def reference(case):
    """float64 gradients, their magnitudes A, and torch's CPU float32 figures -- computed once per case, never modified"""
    if case not in _REF:
        x, hid, w, b, gy = _inputs(case)
        out64, want = _autograd(x, hid, w, b, gy, torch.float64)
        out_mag, mag = _autograd(x.abs(), hid.abs(), w.abs(), b.abs(), gy.abs(), torch.float64)
        _, got32 = _autograd(x, hid, w, b, gy, torch.float32)
        _REF[case] = dict(out=out64, out_mag=out_mag, want=want, mag=mag, torch32=[metric(g, r, a) for g, r, a in zip(got32, want, mag)])
    return _REF[case]


def metric(got, want, mag, scale=1.0):
    """worst |err| / A in units of 2^-24 (``scale``: the factor the output gradient was multiplied by)"""
    err = (got.detach().double().cpu() - want * scale).abs()
    return float((err / (mag * abs(scale)).clamp_min(1e-300)).max()) / UNIT


def run_kernel(case, gy_scale=1.0, need=(True, True, True, True), inputs=None):
    x, hid, w, b, gy = inputs if inputs is not None else _inputs(case)
    ts = [t.to(DEV).requires_grad_(n) for t, n in zip((x, hid, w, b), need)]
    ws, alpha = fused.pack_conv3x3_weight(ts[2])
    out = T._TemporalFusionCore.apply(*ts, dict(ws=ws, alpha=alpha))
    assert tuple(out.shape) == (x.shape[0], x.shape[2], x.shape[3], 256)
    out.backward((gy * gy_scale).to(DEV).permute(0, 2, 3, 1).contiguous())
    torch.cuda.synchronize()
    return out.detach(), [t.grad for t in ts]


def check(case, grads, gy_scale=1.0):
    ref = reference(case)
    figs = [metric(g, r, a, gy_scale) for g, r, a in zip(grads, ref["want"], ref["mag"])]
    print(f"\ncase {case} (grad_output x {gy_scale:g}): " +
          "  ".join(f"{n} {k:.3f}|{t:.3f}" for n, k, t in zip(NAMES, figs, ref["torch32"])))
    for n, g, k, t in zip(NAMES, grads, figs, ref["torch32"]):
        assert bool(torch.isfinite(g).all()), n
        assert k <= max(2.0 * t, 8.0), f"case {case} {n}: {k:.3f} units against torch float32 {t:.3f}"


@pytest.mark.parametrize("case", list(CASES))
def test_gradients_against_float64(case):
    out, grads = run_kernel(case)
    ref = reference(case)
    # the forward it differentiates is the convolution (channel-last), within the split's bound
    fwd = metric(out.permute(0, 3, 1, 2), ref["out"], ref["out_mag"])
    print(f"\ncase {case}: forward {fwd:.3f}")
    assert fwd <= 8.0
    for g, r in zip(grads, ref["want"]):
        assert g.shape == r.shape
    check(case, grads)


@pytest.mark.parametrize("gy_scale", [1e-6, 1e4])
def test_scale_of_the_output_gradient(gy_scale):
    """the image of grad_output takes its power-of-two scale from grad_output's own maximum"""
    _, grads = run_kernel("A", gy_scale=gy_scale)
    check("A", grads, gy_scale)


def test_zero_output_gradient_gives_exact_zeros():
    _, grads = run_kernel("A", gy_scale=0.0)
    for n, g in zip(NAMES, grads):
        assert bool((g == 0).all()) and not bool(torch.isnan(g).any()), n


def test_frozen_weights_skip_the_weight_gradient(monkeypatch):
    calls = []
    real = fused.conv3x3_wgrad
    monkeypatch.setattr(fused, "conv3x3_wgrad", lambda *a, **k: calls.append(1) or real(*a, **k))
    _, grads = run_kernel("A", need=(True, True, False, False))
    assert not calls and grads[2] is None and grads[3] is None
    ref = reference("A")
    for i in (0, 1):
        assert metric(grads[i], ref["want"][i], ref["mag"][i]) <= max(2.0 * ref["torch32"][i], 8.0)
    # only x: one data-gradient launch, none for the hidden half
    convs = []
    real_conv = fused.ConvImage.conv
    monkeypatch.setattr(fused.ConvImage, "conv", lambda self, *a, **k: convs.append(1) or real_conv(self, *a, **k))
    _, grads = run_kernel("A", need=(True, False, False, False))
    assert len(convs) == 2 and grads[1] is None and grads[0] is not None        # the forward and grad_x


def test_inputs_without_grad_skip_the_data_gradients(monkeypatch):
    convs, wg = [], []
    real_conv, real_wg = fused.ConvImage.conv, fused.conv3x3_wgrad
    monkeypatch.setattr(fused.ConvImage, "conv", lambda self, *a, **k: convs.append(1) or real_conv(self, *a, **k))
    monkeypatch.setattr(fused, "conv3x3_wgrad", lambda *a, **k: wg.append(1) or real_wg(*a, **k))
    _, grads = run_kernel("A", need=(False, False, True, True))
    assert len(convs) == 1 and len(wg) == 1                                      # the forward's launch only
    assert grads[0] is None and grads[1] is None
    ref = reference("A")
    for i in (2, 3):
        assert metric(grads[i], ref["want"][i], ref["mag"][i]) <= max(2.0 * ref["torch32"][i], 8.0)


def test_zero_hidden_half_of_the_weights_gives_a_zero_gradient():
    """a zero-initialised W[:, 256:] has no scale to pack its transposed image with: grad_hid is exactly zero, the rest as ever"""
    x, hid, w, b, gy = _inputs("A")
    w = w.clone()
    w[:, 256:] = 0
    _, grads = run_kernel("A", inputs=(x, hid, w, b, gy))
    _, want = _autograd(x, hid, w, b, gy, torch.float64)
    _, mag = _autograd(x.abs(), hid.abs(), w.abs(), b.abs(), gy.abs(), torch.float64)
    _, got32 = _autograd(x, hid, w, b, gy, torch.float32)
    assert bool((grads[1] == 0).all()) and bool((want[1] == 0).all())
    for i in (0, 2, 3):
        fig, t32 = metric(grads[i], want[i], mag[i]), metric(got32[i], want[i], mag[i])
        print(f"\nzero hidden weights: {NAMES[i]} {fig:.3f}|{t32:.3f}")
        assert fig <= max(2.0 * t32, 8.0)


def test_two_backward_runs_are_bit_identical():
    assert fused.wgrad_k_splits(*CASES["E"][:3], 256 + CASES["E"][3]) > 1
    _, g1 = run_kernel("E")
    _, g2 = run_kernel("E")
    for n, a, b in zip(NAMES, g1, g2):
        assert torch.equal(a, b), f"{n}: two runs differ"


# ---------------------------------------------------------------------------------------------------------------- module level
def _encoder():
    torch.manual_seed(7)
    enc = T.RadarBEVTemporalEncoder(embed_dims=256, hidden_dims=64, num_frames=5)
    bev = torch.randn(1, 5, 256, 16, 16)
    gout = torch.randn(1, 5, 256, 16, 16)
    return enc, bev, gout


def _run_encoder(enc, bev, gout, dev, dtype, switch):
    enc = copy.deepcopy(enc).to(device=dev, dtype=dtype)
    enc.fused_conv_grad = switch
    x = bev.to(device=dev, dtype=dtype).clone().requires_grad_()
    out = enc(x)
    out.backward(gout.to(device=dev, dtype=dtype))
    grads = {"input": x.grad, **{n: p.grad for n, p in enc.named_parameters()}}
    return out.detach().double().cpu(), {n: g.detach().double().cpu() for n, g in grads.items()}


def test_encoder_routes_against_float64(monkeypatch):
    enc, bev, gout = _encoder()
    out64, g64 = _run_encoder(enc, bev, gout, "cpu", torch.float64, False)
    calls = []
    real_f, real_b = T.temporal_fusion_forward, T.temporal_fusion_backward
    monkeypatch.setattr(T, "temporal_fusion_forward", lambda *a, **k: calls.append("f") or real_f(*a, **k))
    monkeypatch.setattr(T, "temporal_fusion_backward", lambda *a, **k: calls.append("b") or real_b(*a, **k))
    out_off, g_off = _run_encoder(enc, bev, gout, DEV, torch.float32, False)
    assert not calls, "with the switch off the module must not call the new entry points"
    out_on, g_on = _run_encoder(enc, bev, gout, DEV, torch.float32, True)
    assert calls == ["f", "b"]
    top = float(out64.abs().max())
    print("\nforward: on-off %.3e, on-f64 %.3e, off-f64 %.3e of max %.3e" % (
        float((out_on - out_off).abs().max()), float((out_on - out64).abs().max()), float((out_off - out64).abs().max()), top))
    assert float((out_on - out_off).abs().max()) <= 1e-4 * top
    assert set(g_on) == set(g64)
    for n, want in g64.items():
        big = float(want.abs().max())
        e_on, e_off = float((g_on[n] - want).abs().max()) / big, float((g_off[n] - want).abs().max()) / big
        print(f"  {n}: on {e_on:.3e}  off {e_off:.3e}")
        assert e_on <= max(2.0 * e_off, 1e-5), f"{n}: {e_on:.3e} against the library route's {e_off:.3e}"


def test_no_grad_forward_is_untouched(monkeypatch):
    """under no_grad, or with nothing requiring grad, the module never enters the autograd route"""
    enc, bev, _ = _encoder()
    enc = enc.to(DEV)
    calls = []
    monkeypatch.setattr(T, "temporal_fusion_forward", lambda *a, **k: calls.append("f"))
    with torch.no_grad():
        enc(bev.to(DEV))
    for p in enc.parameters():
        p.requires_grad_(False)
    enc(bev.to(DEV))
    assert not calls
