"""The image backbone's backward on the MI355X (racformer_amd/resnet.py ``fused_grad``; csrc/resnet_bwd.hip): one call of each new
kernel against float64, then Bottleneck blocks, the whole ResNet-50 and the chain into the necks under autograd.

Reference: float64 CPU autograd through tests/resnet_ref.py's functions; tests/resnet_grad_ref.py adds the variant whose ReLUs multiply
by given masks.

Kernel level.  Metric: worst |err| / A in units of 2^-24, A the same sum with every term taken in absolute value.  Criterion, the one
of tests/test_necks_grad_gpu.py: kernel <= max(2 x the figure of torch's CPU float32 autograd on the same inputs, 8).  Cases: the
forward test's groups (1x1 stride 1: 64->64, 64->256, 256->64, 512->2048, 2048->512; 1x1 stride 2: 256->512, 1024->2048; 3x3 stride 1:
64->64, 512->512; 3x3 stride 2: 128->128, 512->512) on input maps 1x1 (1 image), 2x2 (2), 7x11 (2), 16x44 (3): at stride 2 odd and even
inputs onto 1x1, 1x1, 4x6, 8x22; and two channel counts that end inside a ci tile of the weight gradient, on 7x11.  The data gradient runs with and without ``mask`` and ``add`` (a masked element is exactly 0, also
where the mask value is 0); the weight gradient at k_splits = 1, the default and a ragged count, twice at each for equal bits.  Scale:
g x 1e-6, g x 1e4, one image at 1e3 x the others.  One larger case, 6 x 64->64 3x3 on 64x176.  rac_resnet_relu_bwd bitwise.

Blocks, the whole network and the chain: the reference is evaluated with the ReLU decisions of the route's own saved forward tensors
(``resnet.forward_hip_train``) -- a gradient is the gradient of the function that was evaluated -- after requiring that those decisions
differ from the float64 forward's own in at most 16 elements per fixture.  Criterion for every parameter gradient (convolution
weights, BatchNorm weight and bias): err < max(4 x E_ref, 1e-5 x max|want|), E_ref the CPU float32 autograd with the same masks
against float64.  The route never computes the gradient of the first trainable block's input (the images and frozen stages need
none), so the blocks' input gradients are covered at the kernel level and through the blocks in front (``layer2.1``'s input gradient
is what ``layer2.0``'s parameter gradients are made of).  Blocks: ``layer2.0`` + ``layer2.1`` (downsample at stride 2, then none) and
``layer1.0`` with ``frozen_stages=0`` (downsample at stride 1) on 2 x 7x11 and 2 x 16x44 inputs at ResNet-50's widths.

Measured on an MI355X.  Kernels, worst case of each group, kernel | torch's CPU float32 autograd (units of 2^-24):
  dX   1x1 s1 4.21|5.61   1x1 s2 3.43|4.05   3x3 s1 3.34|0.59 (with add)   3x3 s2 3.32|4.72   big 3.99|2.06
  dW   1x1 s1 5.81|1.00   1x1 s2 7.15|1.95   3x3 s1 6.47|3.92   3x3 s2 6.07|1.95   big 3.24|0.59 (k_splits 1), 0.21|0.59 (56), 0.94|0.59 (5)
  db   1x1 s1 2.70|0.79   1x1 s2 1.66|2.60   3x3 s1 1.59|1.59   3x3 s2 1.05|1.64   big 0.48|0.30
  (the dW maxima are the 1x1 and 2x2 maps: sums of one to eight products, at the split's own bound, the floor of 8, with nothing to
  average over.  With three products instead of four the single-product case 512->2048 on 1x1 measured 8.70: the kernel computes
  lo*lo as well.)
  Channel counts that end inside a ci tile: 192->128 dW 2.16|2.93, 160->64 (3x3 stride 2) dW 2.60|5.44.
  g x 1e-6: dW 1.21|5.26, db 0.45|0.93, dX 3.07|1.42; x 1e4: 1.12, 0.50, 1.83.  One image x 1e3: the other images' dX 2.42|1.54.
Modules, largest err | E_ref of the largest element, and the largest err / bound:
  layer2.0 + layer2.1   1.2e-6|8.0e-7, 0.12      layer1.0   1.3e-6|8.3e-7, 0.13
  ResNet-50 37x53       7.1e-6|1.4e-6, 0.71      32x64      5.4e-6|1.5e-6, 0.54      chain into the necks   3.8e-6|3.5e-6, 0.38
  ReLU decisions that differ from float64's: 1 of 556 800 (37x53), 0 of 423 936 (32x64), at most 1 in the block fixtures.

Every pair is printed before it is asserted; RAC_RESNET_GRAD_ERRORS=<file> writes them as JSON (tools/resnet_bench.py --grad --errors
copies them into profiles/resnet_grad_f8.json)."""
import copy
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import necks_ref as NR
import resnet_grad_ref as RG
import resnet_ref as RR
from racformer_amd import ResNet, necks, resnet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNIT = 2.0 ** -24
GROUPS = {"k1s1": (1, 1, [(64, 64), (64, 256), (256, 64), (512, 2048), (2048, 512)]), "k1s2": (1, 2, [(256, 512), (1024, 2048)]),
          "k3s1": (3, 1, [(64, 64), (512, 512)]), "k3s2": (3, 2, [(128, 128), (512, 512)])}
MAPS = [(1, 1, 1), (2, 2, 2), (7, 11, 2), (16, 44, 3)]       # (H, W, images)
CASES = {f"{grp}_{ci}_{co}-{h}x{w}": (k, s, ci, co, h, w, n) for grp, (k, s, chans) in GROUPS.items() for ci, co in chans
         for h, w, n in MAPS}
CASES["big"] = (3, 1, 64, 64, 64, 176, 6)
CASES["ragged128"] = (1, 1, 192, 128, 7, 11, 2)      # a second 128-channel ci tile with half of it past Cin
CASES["ragged64"] = (3, 2, 160, 64, 7, 11, 2)        # the same on the 64 x 64 tiles (weight gradient only: the data gradient wants Cin % 64)
PAIRS = []
_REF = {}


@pytest.fixture(scope="module", autouse=True)
def _error_pairs():
    yield
    path = os.environ.get("RAC_RESNET_GRAD_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump(PAIRS, f, indent=1)


# ------------------------------------------------------------------------------------------------------------------ kernels
def _inputs(case):
    k, s, ci, co, h, w, n = CASES[case]
    ho, wo = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    seed = 6000 + 13 * sorted(CASES).index(case)
    x = torch.from_numpy(RR.syn.rng_normal(seed, (n, ci, h, w)))
    wt = torch.from_numpy(RR.syn.rng_normal(seed + 1, (co, ci, k, k), 1.0 / float(np.sqrt(ci * k * k))))
    g = torch.from_numpy(RR.syn.rng_normal(seed + 2, (n, co, ho, wo)))
    add = torch.from_numpy(RR.syn.rng_normal(seed + 3, (n, ci, h, w)))
    mask = torch.from_numpy(RR.syn.rng_normal(seed + 4, (n, ci, h, w)))
    mask = torch.where(mask.abs() < 0.3, torch.zeros_like(mask), mask)       # positive, negative and exact zeros
    return x, wt, g, add, mask


def _autograd(case, x, wt, g, dtype):
    """(dX, dW, db) of conv(x, wt) + b by torch's CPU autograd in ``dtype``"""
    k, s = CASES[case][:2]
    x, wt = (t.to(dtype).clone().requires_grad_() for t in (x, wt))
    b = torch.zeros(wt.shape[0], dtype=dtype, requires_grad=True)
    F.conv2d(x, wt, b, stride=s, padding=k // 2).backward(g.to(dtype))
    return x.grad, wt.grad, b.grad


def metric(got, want, mag, scale=1.0):
    """worst |err| / A in units of 2^-24 (``scale``: the factor the gradient was multiplied by)"""
    err = (got.detach().double().cpu() - want * scale).abs()
    return float((err / (mag * abs(scale)).clamp_min(1e-300)).max()) / UNIT


def reference(case):
    """float64 gradients, their magnitudes A and torch's CPU float32 results -- computed once per case, never modified"""
    if case not in _REF:
        x, wt, g, add, mask = _inputs(case)
        want = _autograd(case, x, wt, g, torch.float64)
        mag = _autograd(case, x.abs(), wt.abs(), g.abs(), torch.float64)
        t32 = _autograd(case, x, wt, g, torch.float32)
        _REF[case] = dict(want=want, mag=mag, t32=t32, fig32=[metric(a, r, m) for a, r, m in zip(t32, want, mag)])
    return _REF[case]


def judge(what, fig, t32):
    print(f"\n{what}: kernel {fig:.3f} | torch32 {t32:.3f}")
    PAIRS.append(dict(case=what, kernel=fig, torch32=t32))
    assert fig <= max(2.0 * t32, 8.0), f"{what}: {fig:.3f} units against torch float32 {t32:.3f}"


def run_dgrad(case, wt, g, add=None, mask=None):
    k, s, ci, co, h, w, n = CASES[case]
    packed = resnet.pack_conv_weight_t(wt.to(DEV))
    dev = lambda t: t.to(DEV).contiguous() if t is not None else None      # noqa: E731
    out = resnet.conv_dgrad(dev(g), packed, k, s, (h, w), add=dev(add), mask=dev(mask))
    torch.cuda.synchronize()
    return out.cpu()


def run_wgrad(case, g, x, bias=True, k_splits=None):
    k, s = CASES[case][:2]
    dw, db = resnet.conv_wgrad(g.to(DEV).contiguous(), x.to(DEV).contiguous(), k, s, bias=bias, k_splits=k_splits)
    torch.cuda.synchronize()
    return dw.cpu(), (db.cpu() if db is not None else None)


@pytest.mark.parametrize("case", [c for c in CASES if CASES[c][2] % 64 == 0])
def test_conv_dgrad_against_float64(case):
    x, wt, g, add, mask = _inputs(case)
    ref = reference(case)
    want, mag, t32 = ref["want"][0], ref["mag"][0], ref["t32"][0]
    plain = run_dgrad(case, wt, g)
    assert plain.shape == x.shape and plain.is_contiguous() and bool(torch.isfinite(plain).all())
    judge(f"dgrad {case}", metric(plain, want, mag), ref["fig32"][0])
    keep = mask > 0
    for a, m in ((add, None), (None, mask), (add, mask)):
        got = run_dgrad(case, wt, g, a, m)
        w64, m64, r32 = want, mag, t32
        if a is not None:
            w64, m64, r32 = w64 + a.double(), m64 + a.double().abs(), r32 + a
        if m is not None:
            w64, r32 = torch.where(keep, w64, torch.zeros_like(w64)), torch.where(keep, r32, torch.zeros_like(r32))
            assert bool((got[~keep] == 0).all()) and not bool(torch.signbit(got[~keep]).any())      # exactly +0, mask 0 included
            assert bool((mask[~keep] == 0).any()) or mask.numel() < 1000
        judge(f"dgrad {case} add={a is not None} mask={m is not None}", metric(got, w64, m64), metric(r32, w64, m64))


def _ragged(units):
    for k in (3, 5, 7, 4, 2):
        if k <= units and units % k != 0 and (k - 1) * (-(-units // k)) < units:
            return k
    return None


@pytest.mark.parametrize("case", list(CASES))
def test_conv_wgrad_against_float64(case):
    k, s, ci, co, h, w, n = CASES[case]
    x, wt, g, _, _ = _inputs(case)
    ref = reference(case)
    units = n * ((g.shape[2] * g.shape[3] + 31) // 32)
    default = resnet.conv_wgrad_k_splits(n, g.shape[2], g.shape[3], ci, co, k)
    for ks in dict.fromkeys([1, default, _ragged(units)]):
        if ks is None:
            continue
        dw, db = run_wgrad(case, g, x, k_splits=ks)
        assert dw.shape == wt.shape and db.shape == (co,) and bool(torch.isfinite(dw).all()) and bool(torch.isfinite(db).all())
        judge(f"wgrad {case} k_splits={ks} dW", metric(dw, ref["want"][1], ref["mag"][1]), ref["fig32"][1])
        judge(f"wgrad {case} k_splits={ks} db", metric(db, ref["want"][2], ref["mag"][2]), ref["fig32"][2])
        dw2, db2 = run_wgrad(case, g, x, k_splits=ks)
        assert torch.equal(dw2, dw) and torch.equal(db2, db)
        dw3, none = run_wgrad(case, g, x, bias=False, k_splits=ks)
        assert none is None and torch.equal(dw3, dw)


def test_the_big_case_has_many_k_ranges():
    k, s, ci, co, h, w, n = CASES["big"]
    assert resnet.conv_wgrad_k_splits(n, h, w, ci, co, k) > 50 and n * ((h * w + 63) // 64) >= 256


SCALED = "k3s1_64_64-7x11"


@pytest.mark.parametrize("scale", [1e-6, 1e4])
def test_scale_of_the_gradient(scale):
    """g's scales come from its own maxima: per image in the data gradient, per channel and K range in the weight gradient"""
    x, wt, g, _, _ = _inputs(SCALED)
    ref = reference(SCALED)
    dw, db = run_wgrad(SCALED, g * scale, x)
    judge(f"wgrad {SCALED} g x {scale:g} dW", metric(dw, ref["want"][1], ref["mag"][1], scale), ref["fig32"][1])
    judge(f"wgrad {SCALED} g x {scale:g} db", metric(db, ref["want"][2], ref["mag"][2], scale), ref["fig32"][2])
    judge(f"dgrad {SCALED} g x {scale:g}", metric(run_dgrad(SCALED, wt, g * scale), ref["want"][0], ref["mag"][0], scale),
          ref["fig32"][0])


def test_one_large_image_leaves_the_others_alone():
    """One image of g at 1e3 x the others: the data gradient's scale is per image, so the other images keep their accuracy."""
    case = "k3s1_64_64-16x44"
    x, wt, g, _, _ = _inputs(case)
    g = g.clone()
    g[1] *= 1.0e3
    want, mag = _autograd(case, x, wt, g, torch.float64), _autograd(case, x.abs(), wt.abs(), g.abs(), torch.float64)
    t32 = _autograd(case, x, wt, g, torch.float32)
    got = run_dgrad(case, wt, g)
    for name, sel in (("whole batch", slice(None)), ("the other images", [0, 2])):
        judge(f"dgrad one image x1e3, {name}", metric(got[sel], want[0][sel], mag[0][sel]), metric(t32[0][sel], want[0][sel], mag[0][sel]))
    dw, db = run_wgrad(case, g, x)
    judge("wgrad one image x1e3 dW", metric(dw, want[1], mag[1]), metric(t32[1], want[1], mag[1]))
    judge("wgrad one image x1e3 db", metric(db, want[2], mag[2]), metric(t32[2], want[2], mag[2]))


def test_zero_gradient_gives_exact_zeros():
    x, wt, g, _, _ = _inputs(SCALED)
    z = torch.zeros_like(g)
    dw, db = run_wgrad(SCALED, z, x)
    dx = run_dgrad(SCALED, wt, z)
    for name, t in (("dW", dw), ("db", db), ("dX", dx)):
        assert bool((t == 0).all()) and not bool(torch.isnan(t).any()), name


@pytest.mark.parametrize("shape", [(1, 64, 1, 1), (2, 256, 7, 11), (3, 512, 16, 44)])
def test_relu_bwd_is_the_torch_expression_bitwise(shape):
    y, a, b = (torch.from_numpy(RR.syn.rng_normal(6900 + i, shape)) for i in range(3))
    y = torch.where(y.abs() < 0.3, torch.zeros_like(y), y)
    for second in (b, None):
        got = resnet.relu_bwd(y.to(DEV), a.to(DEV), second.to(DEV) if second is not None else None)
        torch.cuda.synchronize()
        want = torch.where(y > 0, a + second if second is not None else a, torch.zeros_like(a))
        assert torch.equal(got.cpu(), want) and not bool(torch.signbit(got.cpu()[y <= 0]).any())


# -------------------------------------------------------------------------------------------------- blocks and the whole network
def shapes_of(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def _masks(m, xd):
    """{block prefix: (t1 > 0, t2 > 0, y > 0)} from the route's own saved forward tensors, and the forward's outputs"""
    with torch.no_grad():
        outs, saved = resnet.forward_hip_train(m, xd)
    torch.cuda.synchronize()
    blocks = resnet.trainable_blocks(m)
    assert len(saved) == len(blocks)
    return {f"layer{i + 1}.{b}": tuple((t > 0).cpu() for t in s[1:]) for (i, b), s in zip(blocks, saved)}, outs


def _mask_differences(masks, own):
    return sum(int((a != b).sum()) for p, ms in masks.items() for a, b in zip(ms, own[p]))


def _reference_grads(fn, sd, names, gouts, dtype):
    """gradients of the parameters ``names`` through fn(sd) -> outputs, in ``dtype``"""
    sd = {k: (v.to(dtype).clone().requires_grad_(k in names) if v.is_floating_point() else v) for k, v in sd.items()}
    outs = fn(sd)
    pairs = [(o, g.to(dtype)) for o, g in zip(outs, gouts) if g is not None and o.requires_grad]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    return {k: sd[k].grad for k in names}


def hold(what, got, want, ref32):
    err = float((got.double().cpu() - want).abs().max())
    e_ref = float((ref32.double() - want).abs().max())
    big = float(want.abs().max())
    print(f"\n{what}: err {err:.3e}  E_ref {e_ref:.3e}  max|want| {big:.3e}")
    PAIRS.append(dict(case=what, err=err, e_ref=e_ref, big=big))
    assert got.shape == want.shape
    assert err < max(4.0 * e_ref, 1e-5 * big), f"{what}: {err:.3e} against E_ref {e_ref:.3e}, max|want| {big:.3e}"


def _run(m, xd, gouts, switch=True, skip=()):
    """forward + backward of a device model; -> (outs, {parameter name: grad})"""
    m.fused_grad = switch
    for p in m.parameters():
        p.grad = None
    assert m.hip_grad_route(xd) == bool(switch) and not m.hip_route(xd)
    outs = m(xd)
    pairs = [(o, g.to(DEV)) for j, (o, g) in enumerate(zip(outs, gouts)) if o.requires_grad and g is not None and j not in skip]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
    torch.cuda.synchronize()
    return [o.detach() for o in outs], {k: p.grad for k, p in m.named_parameters()}


def _mini(kind, hw):
    """A one-stage network of the named blocks behind a patched stem: the stage's input is given directly."""
    h, w = hw
    if kind == "layer2":
        m = ResNet(50, num_stages=2, out_indices=(1,), frozen_stages=1)
        m.load_state_dict(RR.fill_state(shapes_of(m), RR.SEED + 1))
        m.layer1, m.layer2 = nn.Sequential(), nn.Sequential(m.layer2[0], m.layer2[1])
        cin, layer, prefixes = 256, 2, ("layer2.0", "layer2.1")
    else:
        m = ResNet(50, num_stages=1, out_indices=(0,), frozen_stages=0)
        m.load_state_dict(RR.fill_state(shapes_of(m), RR.SEED + 2))
        m.layer1 = nn.Sequential(m.layer1[0])
        cin, layer, prefixes = 64, 1, ("layer1.0",)
    x = torch.from_numpy(RR.syn.rng_normal(6400 + h, (2, cin, h, w))).clamp_min(0.0)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    xd = x.to(DEV)
    m.stem_hip = lambda img: xd

    def fn(sd_, masks=None, own=None):
        t = x.to(next(v for k, v in sd_.items() if k.endswith("conv1.weight")).dtype)
        for p in prefixes:
            t = RG.bottleneck(sd_, p, t, 2 if p == "layer2.0" else 1, (masks or {}).get(p), own)
        return [t]
    return m, sd, fn, prefixes


@pytest.mark.parametrize("kind", ["layer2", "layer1"])
@pytest.mark.parametrize("hw", [(7, 11), (16, 44)])
def test_blocks_against_float64(kind, hw):
    m, sd, fn, prefixes = _mini(kind, hw)
    img = torch.zeros(2, 3, 8, 8, device=DEV)
    masks, _ = _masks(m, img)
    own = {}
    with torch.no_grad():
        out64 = fn({k: v.double() for k, v in sd.items()}, None, own)[0]
    diff = _mask_differences(masks, own)
    print(f"\n{kind} {hw}: {diff} ReLU decisions differ from float64's")
    assert diff <= 16
    gouts = [torch.from_numpy(RR.syn.rng_normal(6500 + hw[0], tuple(out64.shape)))]
    names = [k for k, p in m.named_parameters() if k.startswith(prefixes)]
    want = _reference_grads(lambda s: fn(s, masks), sd, names, gouts, torch.float64)
    ref32 = _reference_grads(lambda s: fn(s, masks), sd, names, gouts, torch.float32)
    outs, grads = _run(m, img, gouts)
    assert float((outs[0].double().cpu() - out64).abs().max()) < 1e-4 * float(out64.abs().max())
    assert set(k for k, g in grads.items() if g is not None) == set(names)
    for k in names:
        hold(f"{kind} {hw} {k}", grads[k], want[k], ref32[k])


@pytest.fixture(scope="module", params=[(37, 53), (32, 64)])
def whole(request):
    hw = request.param
    m = ResNet(50, frozen_stages=1)
    sd = RR.fill_state(shapes_of(m), RR.SEED)
    m.load_state_dict(sd)
    m = m.to(DEV).train()
    x = RR.make_images(hw, norm=False)
    xd = x.to(DEV)
    gouts = [torch.from_numpy(RR.syn.rng_normal(6600 + i, (x.shape[0], 256 * 2 ** i) + s)) for i, s in enumerate(RR.stage_sizes(*hw))]
    outs, grads = _run(m, xd, gouts)
    return dict(hw=hw, m=m, sd=sd, x=x, xd=xd, gouts=gouts, outs=outs, grads=grads)


def test_whole_network_against_float64(whole):
    m, sd, x, gouts = whole["m"], whole["sd"], whole["x"], whole["gouts"]
    masks, _ = _masks(m, whole["xd"])
    own = {}
    with torch.no_grad():
        RG.resnet({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, x.double(), None, own)
    diff = _mask_differences(masks, own)
    print(f"\nResNet-50 {whole['hw']}: {diff} of {sum(a.numel() for ms in masks.values() for a in ms)} ReLU decisions differ")
    assert diff <= 16
    names = [k for k, p in m.named_parameters() if p.requires_grad]
    assert names and all(k.startswith(("layer2", "layer3", "layer4")) for k in names)
    want = _reference_grads(lambda s: RG.resnet(s, x.to(s["conv1.weight"].dtype), masks), sd, names, gouts, torch.float64)
    ref32 = _reference_grads(lambda s: RG.resnet(s, x.to(s["conv1.weight"].dtype), masks), sd, names, gouts, torch.float32)
    for k, g in whole["grads"].items():
        if k in names:
            hold(f"ResNet-50 {whole['hw']} {k}", g, want[k], ref32[k])
        else:
            assert g is None and k.startswith(("conv1", "bn1", "layer1")), k       # the stem and layer1 have no gradient


def test_forward_under_fused_grad_is_the_no_grad_route_bitwise(whole):
    m = whole["m"]
    with torch.no_grad():
        assert m.hip_route(whole["xd"]) and not m.hip_grad_route(whole["xd"])
        plain = m(whole["xd"])
    assert len(plain) == 4
    for a, b in zip(plain, whole["outs"]):
        assert torch.equal(a, b)
    assert [o.requires_grad for o in m(whole["xd"])] == [False, True, True, True]


def test_two_backward_runs_give_the_same_bits(whole):
    _, again = _run(whole["m"], whole["xd"], whole["gouts"])
    for k, g in whole["grads"].items():
        assert (g is None and again[k] is None) or torch.equal(g, again[k]), k


def _count(monkeypatch, name):
    calls, real = [], getattr(resnet, name)
    monkeypatch.setattr(resnet, name, lambda *a, **k: calls.append(1) or real(*a, **k))
    return calls


def test_without_the_switch_training_takes_the_torch_route(whole, monkeypatch):
    wg, dg = _count(monkeypatch, "conv_wgrad"), _count(monkeypatch, "conv_dgrad")
    _, grads = _run(whole["m"], whole["xd"], whole["gouts"], switch=False)
    assert not wg and not dg
    for k, g in whole["grads"].items():
        assert (g is None) == (grads[k] is None), k
    assert bool(torch.isfinite(grads["layer2.0.conv1.weight"]).all())


def test_launch_counts_and_frozen_parameters(whole, monkeypatch):
    """13 blocks behind layer1: 42 convolutions' weight gradients, 2 data gradients per block, conv1's for all but the first block, the
    downsample's for layer3.0 and layer4.0, one ReLU backward at the top."""
    wg, dg, rb = _count(monkeypatch, "conv_wgrad"), _count(monkeypatch, "conv_dgrad"), _count(monkeypatch, "relu_bwd")
    m = copy.deepcopy(whole["m"])
    _, grads = _run(m, whole["xd"], whole["gouts"])
    assert (len(wg), len(dg), len(rb)) == (42, 26 + 12 + 2, 1)
    # layer2 frozen: its 13 weight gradients and every data gradient into and inside it disappear, the rest keeps its bits
    del wg[:], dg[:], rb[:]
    for p in m.layer2.parameters():
        p.requires_grad_(False)
    _, part = _run(m, whole["xd"], whole["gouts"])
    assert (len(wg), len(dg), len(rb)) == (29, 18 + 8 + 1, 1)
    for k, g in part.items():
        if k.startswith(("layer3", "layer4")):
            assert torch.equal(g, grads[k]), k
        else:
            assert g is None, k
    # the BatchNorm affine parameters frozen: every convolution's weight gradient still runs and keeps its bits
    del wg[:], dg[:], rb[:]
    m = copy.deepcopy(whole["m"])
    for mod in m.modules():
        if isinstance(mod, nn.BatchNorm2d):
            for p in mod.parameters():
                p.requires_grad_(False)
    _, part = _run(m, whole["xd"], whole["gouts"])
    assert (len(wg), len(dg), len(rb)) == (42, 40, 1)
    for k, g in part.items():
        if ".conv" in k or "downsample.0" in k:
            assert (g is None and grads[k] is None) or torch.equal(g, grads[k]), k
        else:
            assert g is None, k


def test_frozen_stages_2_saves_and_runs_nothing_of_layer2(whole, monkeypatch):
    m = ResNet(50, frozen_stages=2)
    m.load_state_dict(whole["sd"])
    m = m.to(DEV).train()
    with torch.no_grad():
        _, saved = resnet.forward_hip_train(m, whole["xd"])
    assert len(saved) == 9 and resnet.trainable_blocks(m)[0] == (2, 0) and saved[0][0].shape[1] == 512
    wg, dg = _count(monkeypatch, "conv_wgrad"), _count(monkeypatch, "conv_dgrad")
    outs, grads = _run(m, whole["xd"], whole["gouts"])
    assert (len(wg), len(dg)) == (29, 27) and [o.requires_grad for o in m(whole["xd"])] == [False, False, True, True]
    for k, g in grads.items():
        if k.startswith(("layer3", "layer4")):
            assert torch.equal(g, whole["grads"][k]), k
        else:
            assert g is None, k


def test_a_missing_output_gradient_equals_zeros_bitwise(whole):
    zeros = list(whole["gouts"])
    zeros[2] = torch.zeros_like(zeros[2])
    _, with_zeros = _run(whole["m"], whole["xd"], zeros)
    _, with_none = _run(whole["m"], whole["xd"], whole["gouts"], skip=(2,))
    for k, g in with_zeros.items():
        assert (g is None and with_none[k] is None) or torch.equal(g, with_none[k]), k
    assert not torch.equal(with_zeros["layer3.0.conv1.weight"], whole["grads"]["layer3.0.conv1.weight"])


# ------------------------------------------------------------------------------------------------------------------ chain
def _neck(sd, prefix, xs, outs_of):
    """FPN / CustomFPN in the dtype of its inputs: laterals, top-down nearest upsampling, 3x3 outputs of the levels ``outs_of``"""
    t = lambda k: sd[f"{prefix}.{k}"].to(xs[0].dtype)      # noqa: E731
    lat = [F.conv2d(x, t(f"lateral_convs.{i}.conv.weight"), t(f"lateral_convs.{i}.conv.bias")) for i, x in enumerate(xs)]
    for i in range(len(lat) - 1, 0, -1):
        lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode="nearest")
    return [F.conv2d(lat[i], t(f"fpn_convs.{j}.conv.weight"), t(f"fpn_convs.{j}.conv.bias"), padding=1) for j, i in enumerate(outs_of)]


def test_chain_into_both_necks():
    hw = (32, 64)
    m = ResNet(50, frozen_stages=1)
    fpn = necks.FPN([256, 512, 1024, 2048], 256, 4)
    lss = necks.CustomFPN([1024, 2048], 256, num_outs=1, start_level=0, out_ids=[0])
    sd = RR.fill_state(shapes_of(m), RR.SEED)
    sd.update({f"fpn.{k}": v for k, v in NR.fill_state(shapes_of(fpn), 6700).items()})
    sd.update({f"lss.{k}": v for k, v in NR.fill_state(shapes_of(lss), 6701).items()})
    m.load_state_dict({k: v for k, v in sd.items() if not k.startswith(("fpn.", "lss."))})
    fpn.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("fpn.")})
    lss.load_state_dict({k[4:]: v for k, v in sd.items() if k.startswith("lss.")})
    m, fpn, lss = m.to(DEV).train(), fpn.to(DEV).train(), lss.to(DEV).train()
    m.fused_grad = fpn.fused_grad = lss.fused_grad = True
    x = RR.make_images(hw, norm=False)
    xd = x.to(DEV)
    sizes = RR.stage_sizes(*hw)
    gouts = [torch.from_numpy(RR.syn.rng_normal(6800 + i, (x.shape[0], 256) + s)) for i, s in enumerate(sizes + [sizes[2]])]
    masks, _ = _masks(m, xd)
    own = {}
    with torch.no_grad():
        RG.resnet({k: v.double() if v.is_floating_point() else v for k, v in sd.items()}, x.double(), None, own)
    assert _mask_differences(masks, own) <= 16

    def fn(s):
        stages = RG.resnet(s, x.to(s["conv1.weight"].dtype), masks)
        return _neck(s, "fpn", stages, [0, 1, 2, 3]) + _neck(s, "lss", stages[2:], [0])
    names = [k for k, p in m.named_parameters() if p.requires_grad]
    want = _reference_grads(fn, sd, names, gouts, torch.float64)
    ref32 = _reference_grads(fn, sd, names, gouts, torch.float32)
    assert m.hip_grad_route(xd)
    stages = m(xd)
    assert fpn.hip_grad_route(list(stages)) and lss.hip_grad_route(list(stages[2:]))
    outs = list(fpn(list(stages))) + [lss(list(stages[2:]))]
    outs = [o[0] if isinstance(o, (tuple, list)) else o for o in outs]
    torch.autograd.backward(outs, [g.to(DEV) for g in gouts])
    torch.cuda.synchronize()
    for k, p in m.named_parameters():
        if k in names:
            hold(f"chain {k}", p.grad, want[k], ref32[k])
        else:
            assert p.grad is None, k
