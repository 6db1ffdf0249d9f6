"""The image necks on the GPU (racformer_amd/necks.py, csrc/fpn_lateral.hip, rac_conv3x3_cf_fwd): the lateral kernel and the
channel-first output convolution against float64, both modules against the reference's golden and float64, the pregrouped layout
against the oracle's regroup, reproducibility and capture.

Tolerance: the project's rule for split-precision convolutions (tests/test_decoder_gpu.py:126),
    err < max(4 * E_ref, 3e-6 * max|want|) + 1e-6,
E_ref = the error of a CPU fp32 F.conv2d (plus add) on the same inputs against float64, measured per case.  Every (E_ref, err) pair
is printed; RAC_NECKS_ERRORS=<file> writes them as JSON (tools/necks_bench.py --errors copies them into the record)."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import necks_ref as NR
from oracle import restate as R
from racformer_amd import fused, necks
from racformer_amd.fpn_writer import output_conv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = []


@pytest.fixture(scope="module", autouse=True)
def _error_pairs():
    yield
    path = os.environ.get("RAC_NECKS_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump(PAIRS, f, indent=1)


def within_rule(what, got, want, fp32, stages=1):
    """The rule above (``stages`` split-precision stages in a row: each gets the rule's allowance, in units of the final output)."""
    err = (got.double() - want).abs().max().item()
    e_ref = (fp32.double() - want).abs().max().item()
    wmax = float(want.abs().max())
    print(f"{what}: E_ref={e_ref:.3e} err={err:.3e} max|want|={wmax:.3e}")
    PAIRS.append(dict(case=what, e_ref=e_ref, err=err, want_max=wmax))
    assert err < stages * (max(4 * e_ref, 3e-6 * wmax) + 1e-6), (what, err, e_ref, wmax)


def lateral_weights(cin, seed):
    w = torch.from_numpy(NR.syn.rng_normal(seed, (256, cin, 1, 1), 1.0 / float(np.sqrt(cin))))
    b = torch.from_numpy(NR.syn.rng_normal(seed + 1, (256,), 0.1))
    return w, b


def run_lateral(x, w, b, top):
    packed = necks.pack_lateral_weight(w.to(DEV))
    out = necks.fpn_lateral(x.to(DEV), packed, b.to(DEV) if b is not None else None, top.to(DEV) if top is not None else None)
    torch.cuda.synchronize()
    return out.cpu()


def fp32_lateral(x, w, b, top):
    y = F.conv2d(x, w, b)
    return y if top is None else y + F.interpolate(top, size=x.shape[2:], mode="nearest")


TOPS = {(8, 22): [None, (4, 11)], (7, 11): [None, (4, 6), (1, 1)], (1, 1): [None, (1, 1)], (16, 44): [None, (8, 22)]}


@pytest.mark.parametrize("cin", [32, 96, 256, 2048])
@pytest.mark.parametrize("hw,images", [((8, 22), 3), ((7, 11), 2), ((1, 1), 1), ((16, 44), 6)])
def test_lateral_kernel_vs_float64(cin, hw, images):
    """One chunk, an odd chunk count, the common case and the deepest K, on maps of 176 pixels (two tiles, the second ragged), 77
    (odd: 4-byte loads), one pixel and 704 (whole tiles, 16-byte loads); with and without bias; without top, with a top of exactly
    half the size and with ragged ones; signed normal and post-ReLU inputs."""
    w, b = lateral_weights(cin, 10 * cin + hw[0])
    for kind in ("signed", "relu"):
        x = torch.from_numpy(NR.syn.rng_normal(cin + 7 * hw[1] + (kind == "relu"), (images, cin) + hw))
        if kind == "relu":
            x = x.clamp_min(0.0)
        core = torch.einsum("oc,nchw->nohw", w.double().reshape(256, cin), x.double())
        for top_hw in TOPS[hw]:
            top = None if top_hw is None else torch.from_numpy(NR.syn.rng_normal(cin + 3, (images, 256) + top_hw))
            for bias in (b, None):
                want = core if bias is None else core + bias.double()[None, :, None, None]
                if top is not None:
                    want = want + NR.upsample_nearest(top.double(), hw)
                got = run_lateral(x, w, bias, top)
                assert got.shape == (images, 256) + hw and got.is_contiguous()
                within_rule(f"lateral Cin={cin} {hw[0]}x{hw[1]}x{images} {kind} top={top_hw} bias={bias is not None}", got, want,
                            fp32_lateral(x, w, bias, top))


@pytest.mark.parametrize("hw,top_hw", [((64, 176), (32, 88)), ((65, 175), (33, 88))])
def test_lateral_kernel_128_pixel_tiles_vs_float64(hw, top_hw):
    """From 256 tiles of 128 pixels on (a workgroup per CU) the launcher takes the 128-pixel tile; below, as in every case above,
    the 64-pixel one.  Six images of 64 x 176 (528 tiles, 16-byte loads) and of 65 x 175 (534 tiles, odd: 4-byte loads, a ragged
    last tile and a ragged top), two K steps."""
    cin, images = 64, 6
    assert necks.lateral_tile_pixels(images, *hw)[0] == 128 and necks.lateral_tile_pixels(6, 16, 44)[0] == 64
    w, b = lateral_weights(cin, 300 + hw[0])
    x = torch.from_numpy(NR.syn.rng_normal(301 + hw[0], (images, cin) + hw)).clamp_min(0.0)
    top = torch.from_numpy(NR.syn.rng_normal(302, (images, 256) + top_hw))
    for t in (top, None):
        want = NR.lateral(x, w, b, None if t is None else t.double())
        within_rule(f"lateral 128-pixel tiles {hw[0]}x{hw[1]}x{images} top={t is not None}", run_lateral(x, w, b, t), want,
                    fp32_lateral(x, w, b, t))


def test_lateral_kernel_one_large_pixel():
    """A single pixel at 1e3 times the rest: the activation scale is per pixel, so its neighbours keep their accuracy."""
    cin, hw, images = 256, (8, 22), 3
    w, b = lateral_weights(cin, 77)
    x = torch.from_numpy(NR.syn.rng_normal(78, (images, cin) + hw))
    x[1, :, 3, 5] *= 1.0e3
    top = torch.from_numpy(NR.syn.rng_normal(79, (images, 256, 4, 11)))
    want = NR.lateral(x, w, b, top.double())
    got = run_lateral(x, w, b, top)
    within_rule("lateral one pixel x1e3, whole output", got, want, fp32_lateral(x, w, b, top))
    keep = torch.ones(images, 1, *hw, dtype=torch.bool)
    keep[1, :, 3, 5] = False
    keep = keep.expand_as(want)
    # the other pixels under the rule with THEIR maximum
    fp = fp32_lateral(x, w, b, top)
    within_rule("lateral one pixel x1e3, the other pixels", got[keep], want[keep], fp[keep])


def test_lateral_kernel_all_zero_image_is_bias_plus_top_bitwise():
    cin, hw, images = 96, (7, 11), 2
    w, b = lateral_weights(cin, 81)
    x = torch.from_numpy(NR.syn.rng_normal(82, (images, cin) + hw))
    x[1] = 0.0
    top = torch.from_numpy(NR.syn.rng_normal(83, (images, 256, 4, 6)))
    got = run_lateral(x, w, b, top)
    want1 = b[None, :, None, None] + F.interpolate(top[1:2], size=hw, mode="nearest")
    assert torch.equal(got[1:2], want1)
    got_nb = run_lateral(x, w, None, None)
    assert torch.equal(got_nb[1], torch.zeros(256, *hw))


@pytest.mark.parametrize("hw", [(16, 44), (2, 6)])
def test_conv3x3_cf_vs_float64_and_channel_last_bits(hw):
    images = 6
    wt = torch.from_numpy(NR.syn.rng_normal(91, (256, 256, 3, 3), 1.0 / 48.0))
    b = torch.from_numpy(NR.syn.rng_normal(92, (256,), 0.1))
    x = torch.from_numpy(NR.syn.rng_normal(93 + hw[0], (images, 256) + hw))
    want = F.conv2d(x.double(), wt.double(), b.double(), padding=1)
    packed = fused.pack_conv3x3_weight(wt.to(DEV))
    xd, bd = x.to(DEV), b.to(DEV)
    got = output_conv(xd, packed, bd, "test")
    assert got.shape == (images, 256) + hw and got.is_contiguous()
    within_rule(f"conv3x3_cf {hw[0]}x{hw[1]}x{images}", got.cpu(), want, F.conv2d(x, wt, b, padding=1))
    img = fused.ConvImage(images, hw[0], hw[1], 256, xd.device).begin([xd]).pack(xd, 0)
    cl = img.conv(packed[0], packed[1], bias=bd)                       # [n, H, W, 256] (rac_conv3x3_fwd)
    assert torch.equal(got, cl.permute(0, 3, 1, 2))


# ------------------------------------------------------------------------------------------------------------------ modules
def shapes_of(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


@pytest.fixture(scope="module")
def lss(golden_dir):
    g = np.load(os.path.join(golden_dir, "necks_small.npz"))
    m = necks.CustomFPN(NR.LSS["channels"], 256, num_outs=1, start_level=0, out_ids=[0]).eval()
    sd = NR.fill_state(shapes_of(m), int(g["lss:weight_seed"]))
    m.load_state_dict(sd)
    xs = [torch.from_numpy(g["lss:in0"]), torch.from_numpy(g["lss:in1"])]
    with torch.no_grad():
        fp32 = m(xs)
    return dict(g=g, m=m.to(DEV), xs=xs, want=NR.custom_fpn(sd, xs), fp32=fp32)


@pytest.fixture(scope="module")
def fpn4(golden_dir):
    g = np.load(os.path.join(golden_dir, "necks_small.npz"))
    m = necks.FPN(NR.FPN4["channels"], 256, 4, num_cams=3).eval()
    sd = NR.fill_state(shapes_of(m), int(g["fpn:weight_seed"]))
    m.load_state_dict(sd)
    xs = NR.make_inputs(int(g["fpn:input_seed"]), NR.FPN4["images"], NR.FPN4["channels"], NR.FPN4["maps"], relu=True)
    with torch.no_grad():
        fp32 = m(xs)
    return dict(g=g, m=m.to(DEV), xs=xs, want=NR.fpn(sd, xs), fp32=fp32)


def test_custom_fpn_vs_golden_and_float64(lss):
    m, xs = lss["m"], [x.to(DEV) for x in lss["xs"]]
    with torch.no_grad():
        assert m.hip_route(xs)
        got = m(xs)
    assert got.shape == (2, 256, 7, 11) and got.is_contiguous() and got.dtype == torch.float32
    within_rule("CustomFPN vs float64", got.cpu(), lss["want"], lss["fp32"], stages=2)
    gold = torch.from_numpy(lss["g"]["lss:out"])
    # the golden is itself an fp32 result: its own distance from float64 joins the allowance
    e_gold = (gold.double() - lss["want"]).abs().max().item()
    e_ref = (lss["fp32"].double() - lss["want"]).abs().max().item()
    err = (got.cpu() - gold).abs().max().item()
    print(f"CustomFPN vs golden: err={err:.3e} e_gold={e_gold:.3e} E_ref={e_ref:.3e}")
    assert err < 2 * (max(4 * e_ref, 3e-6 * float(lss["want"].abs().max())) + 1e-6) + e_gold


def test_fpn_vs_golden_and_float64(fpn4):
    m, xs = fpn4["m"], [x.to(DEV) for x in fpn4["xs"]]
    ch = NR.FPN4_CHANNELS
    with torch.no_grad():
        assert m.hip_route(xs)
        got = m(xs)
    assert isinstance(got, tuple) and len(got) == 4
    for i, (a, want, fp32) in enumerate(zip(got, fpn4["want"], fpn4["fp32"])):
        assert a.shape == (6, 256) + NR.FPN4["maps"][i] and a.is_contiguous()
        within_rule(f"FPN level {i} vs float64", a.cpu(), want, fp32, stages=2)
        gold = torch.from_numpy(fpn4["g"][f"fpn:out{i}"])
        e_gold = (gold.double() - want[:, ch]).abs().max().item()
        e_ref = (fp32.double() - want).abs().max().item()
        err = (a.cpu()[:, ch] - gold).abs().max().item()
        print(f"FPN level {i} vs golden: err={err:.3e} e_gold={e_gold:.3e} E_ref={e_ref:.3e}")
        assert err < 2 * (max(4 * e_ref, 3e-6 * float(want.abs().max())) + 1e-6) + e_gold


def test_fpn_pregrouped_vs_oracle_regroup_and_own_forward(fpn4):
    """``forward_pregrouped`` against the ORACLE's regroup of the float64 outputs under the rule, and against the regroup of
    ``forward``'s own outputs BITWISE: the two epilogues store the same fma(acc, unscale, bias) of the same accumulators."""
    m, xs = fpn4["m"], [x.to(DEV) for x in fpn4["xs"]]
    cams = m.num_cams
    with torch.no_grad():
        grouped = m.forward_pregrouped(xs)
        plain = m(xs)
    for i, (gq, want, fp32, p) in enumerate(zip(grouped, fpn4["want"], fpn4["fp32"], plain)):
        h, w = NR.FPN4["maps"][i]
        assert gq.shape == (6 // cams * 4, cams, h, w, 64)
        within_rule(f"FPN pregrouped level {i}", gq.cpu(), R.regroup_pyramid([want[None]], cams)[0], R.regroup_pyramid([fp32[None]], cams)[0],
                    stages=2)
        assert torch.equal(gq.cpu(), R.regroup_pyramid([p.cpu()[None]], cams)[0])


def test_custom_fpn_output_feeds_depth_net(lss):
    from racformer_amd.depth_net import DepthNet
    m, xs = lss["m"], [x.to(DEV) for x in lss["xs"]]
    net = DepthNet(256, 256, 64, 24, use_dcn=False).eval().to(DEV)
    mlp = torch.randn(1, 2, 9, device=DEV)
    with torch.no_grad():
        x = m(xs)
        assert x.is_contiguous() and x.dtype == torch.float32 and x.shape[1] == 256 and x.is_cuda
        assert net.hip_route(x, mlp)


def test_training_and_unfused_take_the_torch_route(lss):
    m, xs = lss["m"], [x.to(DEV) for x in lss["xs"]]
    assert not m.hip_route(xs)                       # gradients enabled, parameters require them
    with torch.no_grad():
        assert m.hip_route(xs) and not m.hip_route([x.double() for x in xs]) and not m.hip_route(lss["xs"])
        m.fused = False
        try:
            assert not m.hip_route(xs)
            got = m(xs)
        finally:
            m.fused = True
    assert (got.cpu().double() - lss["want"]).abs().max().item() < 1e-4 * float(lss["want"].abs().max())


# ------------------------------------------------------------------------------------------ reproducibility and capture
def test_two_eager_runs_give_the_same_bits(lss, fpn4):
    with torch.no_grad():
        xs = [x.to(DEV) for x in lss["xs"]]
        assert torch.equal(lss["m"](xs), lss["m"](xs))
        xs = [x.to(DEV) for x in fpn4["xs"]]
        for a, b in zip(fpn4["m"](xs), fpn4["m"](xs)):
            assert torch.equal(a, b)


def test_captured_custom_fpn_replays_the_eager_bits(lss):
    m, xs = lss["m"], [x.to(DEV) for x in lss["xs"]]
    with torch.no_grad():
        eager = m(xs).clone()
        torch.cuda.synchronize()
        try:
            with fused.scratch_namespace("necks-capture-test"):
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    m(xs)                                  # (allocates the namespace's scratch outside the capture)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    captured = m(xs)
            for _ in range(2):
                captured.zero_()
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(captured, eager)
        finally:
            fused.release_scratch("necks-capture-test")
