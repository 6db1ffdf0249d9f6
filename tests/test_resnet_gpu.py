"""The image backbone on the GPU (racformer_amd/resnet.py, csrc/resnet.hip): the Bottleneck convolution kernel at the smallest shapes
at which each of its paths can go wrong, the stem, single blocks, the whole ``ResNet(50)``, the chain into the necks, routing,
reproducibility and capture -- all against float64 torch (tests/resnet_ref.py; there is no golden from the reference, whose tree has
no ResNet-50).

Tolerance: the project's rule for split-precision convolutions (tests/test_decoder_gpu.py:126, tests/test_necks_gpu.py:36),
    err < stages * (max(4 * E_ref, 3e-6 * max|want|) + 1e-6),
E_ref = the error of the CPU fp32 restatement against float64 on the same inputs, measured per case; ``stages`` = the number of
convolutions on the longest path from the test's input to the checked output: 1 for a kernel case, 3 for a block, 10 / 22 / 40 / 49
for the four stage outputs of the network, and 49 + 2 for every neck output (the top-down path carries the deepest stage into every
level).  Every (E_ref, err) pair is printed; RAC_RESNET_ERRORS=<file> writes them as JSON.

The kernel's activation scale is per image (not per pixel): the large-value case is one image, not one pixel.  Its launcher takes 256,
128 or 64 output channels per workgroup by the workgroup count (``resnet.conv_tile_channels``): the small maps of the kernel cases sit
on the 64 side but for the widest outputs, so ``test_conv_kernel_tile_widths`` runs each width on both sides of its switch."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import necks_ref as NR
import resnet_ref as RR
from racformer_amd import ResNet, fused, necks, resnet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAIRS = []
STAGES = (10, 22, 40, 49)


@pytest.fixture(scope="module", autouse=True)
def _error_pairs():
    yield
    path = os.environ.get("RAC_RESNET_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump(PAIRS, f, indent=1)


def within_rule(what, got, want, fp32, stages=1, group=None):
    err = (got.double() - want).abs().max().item()
    e_ref = (fp32.double() - want).abs().max().item()
    wmax = float(want.abs().max())
    print(f"{what}: E_ref={e_ref:.3e} err={err:.3e} max|want|={wmax:.3e} stages={stages}")
    PAIRS.append(dict(case=what, group=group or what.split(" ")[0], e_ref=e_ref, err=err, want_max=wmax, stages=stages))
    assert err < stages * (max(4 * e_ref, 3e-6 * wmax) + 1e-6), (what, err, e_ref, wmax)


# -------------------------------------------------------------------------------------------------------- the convolution kernel
GROUPS = {"1x1s1": (1, 1, [(64, 64), (64, 256), (256, 64), (512, 2048), (2048, 512)]),
          "1x1s2": (1, 2, [(256, 512), (1024, 2048)]),
          "3x3s1": (3, 1, [(64, 64), (512, 512)]),
          "3x3s2": (3, 2, [(128, 128), (512, 512)])}
MAPS = [((1, 1), 1), ((2, 2), 2), ((7, 11), 2), ((16, 44), 3)]
KERNEL_CASES = [(g, cin, cout, hw, n) for g, (_, _, pairs) in GROUPS.items() for cin, cout in pairs for hw, n in MAPS]


def conv_weights(cin, cout, k, seed):
    w = torch.from_numpy(RR.syn.rng_normal(seed, (cout, cin, k, k), float(np.sqrt(2.0 / (cin * k * k)))))
    b = torch.from_numpy(RR.syn.rng_normal(seed + 1, (cout,), 0.1))
    return w, b


def run_conv(x, w, b, k, s, res, relu):
    packed = resnet.pack_conv_weight(w.to(DEV))
    out = resnet.conv_fwd(x.to(DEV), packed, b.to(DEV) if b is not None else None, k, s, res.to(DEV) if res is not None else None, relu)
    torch.cuda.synchronize()
    return out.cpu()


def epilogue(core, b, res, relu):
    y = core if b is None else core + b.to(core.dtype)[None, :, None, None]
    if res is not None:
        y = y + res.to(core.dtype)
    return F.relu(y) if relu else y


@pytest.mark.parametrize("cin,cout,k,s,hw,images,width", [(64, 256, 1, 1, (64, 64), 4, 256), (64, 256, 1, 1, (64, 64), 3, 128),
                                                          (64, 256, 1, 1, (32, 63), 3, 64), (128, 128, 3, 2, (64, 64), 16, 128),
                                                          (128, 128, 3, 2, (64, 63), 15, 64), (64, 256, 3, 1, (31, 33), 16, 256)])
def test_conv_kernel_tile_widths(cin, cout, k, s, hw, images, width):
    """Each workgroup width on both sides of its switch (256 workgroups): 256 pixel tiles x one 256-channel block against 192 x two
    128-channel blocks and 96 x four 64-channel blocks; 256 tiles x one 128-channel block against 240 x two 64-channel blocks; and the
    3x3 / stride 1 on 16 tiles (the last one ragged) x 16 images x one 256-channel block."""
    ho, wo = resnet.conv_out_size(hw[0], hw[1], k, s)
    assert resnet.conv_tile_channels(cout, images, ho, wo)[0] == width
    w, b = conv_weights(cin, cout, k, 31 + images)
    x = torch.from_numpy(RR.syn.rng_normal(32 + images, (images, cin) + hw)).clamp_min(0.0)
    res = torch.from_numpy(RR.syn.rng_normal(33, (images, cout, ho, wo)))
    want = epilogue(F.conv2d(x.double(), w.double(), None, stride=s, padding=k // 2), b, res, True)
    fp32 = epilogue(F.conv2d(x, w, None, stride=s, padding=k // 2), b, res, True)
    within_rule(f"tiles {width}-wide {cin}->{cout} k{k}s{s} {hw[0]}x{hw[1]}x{images}", run_conv(x, w, b, k, s, res, True), want, fp32,
                group="tile-width")


@pytest.mark.parametrize("group,cin,cout,hw,images", KERNEL_CASES)
def test_conv_kernel_vs_float64(group, cin, cout, hw, images):
    """Per group the channel pairs of the issue (one K chunk, several, the widest output, the deepest K) on maps of one pixel (every
    tap but the centre is padding), 2 x 2 (stride 2 gives one pixel), 7 x 11 (odd: a ragged tile, the stride-2 last row and column) and
    16 x 44 (whole tiles); with and without residual, ReLU on and off; signed normal and post-ReLU inputs."""
    k, s, _ = GROUPS[group]
    w, b = conv_weights(cin, cout, k, 7 * cin + cout + k)
    ho, wo = resnet.conv_out_size(hw[0], hw[1], k, s)
    res = torch.from_numpy(RR.syn.rng_normal(cin + cout + hw[0], (images, cout, ho, wo)))
    for kind in ("signed", "relu"):
        x = torch.from_numpy(RR.syn.rng_normal(cin + 3 * hw[1] + (kind == "relu"), (images, cin) + hw))
        if kind == "relu":
            x = x.clamp_min(0.0)
        core64 = F.conv2d(x.double(), w.double(), None, stride=s, padding=k // 2)
        core32 = F.conv2d(x, w, None, stride=s, padding=k // 2)
        for r, relu, bias in ((None, True, b), (res, True, b), (res, False, b), (None, False, None)):
            got = run_conv(x, w, bias, k, s, r, relu)
            assert got.shape == (images, cout, ho, wo) and got.is_contiguous()
            within_rule(f"{group} {cin}->{cout} {hw[0]}x{hw[1]}x{images} {kind} res={r is not None} relu={relu} bias={bias is not None}",
                        got, epilogue(core64, bias, r, relu), epilogue(core32, bias, r, relu))


@pytest.mark.parametrize("group,cin,cout", [("1x1s1", 64, 256), ("1x1s2", 256, 512), ("3x3s1", 64, 64), ("3x3s2", 128, 128)])
def test_conv_kernel_all_zero_image_is_relu_of_bias_plus_residual_bitwise(group, cin, cout):
    k, s, _ = GROUPS[group]
    hw, images = (7, 11), 2
    w, b = conv_weights(cin, cout, k, 11)
    ho, wo = resnet.conv_out_size(hw[0], hw[1], k, s)
    res = torch.from_numpy(RR.syn.rng_normal(12, (images, cout, ho, wo)))
    x = torch.from_numpy(RR.syn.rng_normal(13, (images, cin) + hw))
    x[1] = 0.0
    got = run_conv(x, w, b, k, s, res, True)
    assert torch.equal(got[1], F.relu(b[:, None, None] + res[1]))
    got = run_conv(x, w, b, k, s, None, False)
    assert torch.equal(got[1], b[:, None, None].expand(cout, ho, wo))
    got = run_conv(torch.zeros_like(x), w, None, k, s, None, True)
    assert torch.equal(got, torch.zeros(images, cout, ho, wo))


@pytest.mark.parametrize("group,cin,cout", [("1x1s1", 256, 64), ("1x1s2", 256, 512), ("3x3s1", 64, 64), ("3x3s2", 128, 128)])
def test_conv_kernel_one_large_image(group, cin, cout):
    """One image at 1e3 times the others: the activation scale is per image, so the others stay under the rule with THEIR maximum."""
    k, s, _ = GROUPS[group]
    hw, images = (7, 11), 3
    w, b = conv_weights(cin, cout, k, 21)
    x = torch.from_numpy(RR.syn.rng_normal(22, (images, cin) + hw))
    x[1] *= 1.0e3
    want = epilogue(F.conv2d(x.double(), w.double(), None, stride=s, padding=k // 2), b, None, True)
    fp32 = epilogue(F.conv2d(x, w, None, stride=s, padding=k // 2), b, None, True)
    got = run_conv(x, w, b, k, s, None, True)
    within_rule(f"{group} one image x1e3, whole output", got, want, fp32, group="large-image")
    within_rule(f"{group} one image x1e3, the other images", got[[0, 2]], want[[0, 2]], fp32[[0, 2]], group="large-image")


# ---------------------------------------------------------------------------------------------------------------------- modules
def shapes_of(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


@pytest.fixture(scope="module")
def net():
    m = ResNet(50).eval()
    sd = RR.fill_state(shapes_of(m), RR.SEED)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV), sd


@pytest.fixture(scope="module")
def whole(net):
    """Float64 and fp32 restatements of the whole network on the two test images, computed once."""
    _, sd = net
    out = {}
    for hw in ((37, 53), (32, 64)):
        x = RR.make_images(hw, norm=False)
        out[hw] = dict(x=x, want=RR.resnet(sd, x.double()), fp32=RR.resnet(sd, x))
    return out


@pytest.mark.parametrize("hw", [(37, 53), (32, 64), (7, 9), (1, 1)])
@pytest.mark.parametrize("norm", [True, False])
def test_stem_vs_float64(net, hw, norm):
    """[0, 255]-like BGR values with ``input_norm`` set, plain normal input without; against float64 after the pool."""
    m, sd = net
    x = RR.make_images(hw, norm)
    cfg = RR.NORM if norm else None
    want, fp32 = RR.stem(sd, x.double(), cfg), RR.stem(sd, x, cfg)
    m.input_norm = cfg
    try:
        with torch.no_grad():
            got = m.stem_hip(x.to(DEV)).clone()
    finally:
        m.input_norm = None
    assert tuple(got.shape) == (x.shape[0], 64) + resnet.stem_sizes(*hw)[1] == tuple(want.shape)
    within_rule(f"stem {hw[0]}x{hw[1]}x{x.shape[0]} norm={norm}", got.cpu(), want, fp32)


@pytest.mark.parametrize("stage,block,cin", [(0, 0, 64), (1, 0, 256), (1, 1, 512)])
def test_single_block_vs_float64(net, stage, block, cin):
    """layer1.0 (stride 1 with downsample), layer2.0 (stride 2 with downsample), layer2.1 (identity) on 7 x 11 x 2."""
    m, sd = net
    x = torch.from_numpy(RR.syn.rng_normal(40 + cin, (2, cin, 7, 11))).clamp_min(0.0)
    p, stride = f"layer{stage + 1}.{block}", (RR.STRIDES[stage] if block == 0 else 1)
    want, fp32 = RR.bottleneck(sd, p, x.double(), stride), RR.bottleneck(sd, p, x, stride)
    with torch.no_grad():
        got = m.block_hip(stage, block, x.to(DEV))
    assert tuple(got.shape) == tuple(want.shape) and got.is_contiguous()
    within_rule(f"block {p} 7x11x2", got.cpu(), want, fp32, stages=3)


@pytest.mark.parametrize("hw", [(37, 53), (32, 64)])
def test_whole_resnet50_vs_float64(net, whole, hw):
    m, _ = net
    x = whole[hw]["x"].to(DEV)
    assert not m.hip_route(x)                      # gradients enabled, parameters require them
    with torch.no_grad():
        assert m.hip_route(x)
        got = m(x)
    assert isinstance(got, tuple) and len(got) == 4
    for i, (g, want, fp32, size) in enumerate(zip(got, whole[hw]["want"], whole[hw]["fp32"], RR.stage_sizes(*hw))):
        assert tuple(g.shape) == (2, 256 * 2 ** i) + size and g.is_contiguous() and g.dtype == torch.float32 and g.is_cuda
        within_rule(f"resnet50 {hw[0]}x{hw[1]} stage {i}", g.cpu(), want, fp32, stages=STAGES[i])


def test_chain_into_the_necks(net, whole):
    m, _ = net
    hw = (37, 53)
    w = whole[hw]
    fpn = necks.FPN([256, 512, 1024, 2048], 256, 4, num_cams=2).eval()
    lss = necks.CustomFPN([1024, 2048], 256, num_outs=1, start_level=0, out_ids=[0]).eval()
    sd_fpn, sd_lss = NR.fill_state(shapes_of(fpn), 71), NR.fill_state(shapes_of(lss), 72)
    fpn.load_state_dict(sd_fpn)
    lss.load_state_dict(sd_lss)
    want_fpn, want_lss = NR.fpn(sd_fpn, w["want"]), NR.custom_fpn(sd_lss, w["want"][2:])
    with torch.no_grad():
        fp32_fpn, fp32_lss = fpn(w["fp32"]), lss(w["fp32"][2:])
        fpn, lss = fpn.to(DEV), lss.to(DEV)
        feats = m(w["x"].to(DEV))
        assert fpn.hip_route(feats) and lss.hip_route(feats[2:])
        got_fpn, got_lss = fpn(feats), lss(feats[2:])
        grouped = fpn.forward_pregrouped(feats)
    for i in range(4):
        within_rule(f"resnet50->FPN level {i}", got_fpn[i].cpu(), want_fpn[i], fp32_fpn[i], stages=STAGES[3] + 2, group="chain")
        assert tuple(grouped[i].shape) == (4, 2) + tuple(feats[i].shape[2:]) + (64,)
    within_rule("resnet50->CustomFPN", got_lss.cpu(), want_lss, fp32_lss, stages=STAGES[3] + 2, group="chain")


def test_routing(net, whole):
    m, _ = net
    hw = (32, 64)
    x = whole[hw]["x"].to(DEV)
    assert not m.hip_route(x)
    with torch.no_grad():
        assert m.hip_route(x) and not m.hip_route(x.double()) and not m.hip_route(whole[hw]["x"])
        m.fused = False
        try:
            assert not m.hip_route(x)
            got = m(x)
        finally:
            m.fused = True
    for g, want in zip(got, whole[hw]["want"]):
        assert (g.cpu().double() - want).abs().max().item() < 1e-4 * float(want.abs().max())


# ------------------------------------------------------------------------------------------ reproducibility and capture
def test_two_eager_runs_give_the_same_bits(net, whole):
    m, _ = net
    x = whole[(37, 53)]["x"].to(DEV)
    with torch.no_grad():
        a, b = m(x), m(x)
    for u, v in zip(a, b):
        assert u.data_ptr() != v.data_ptr() and torch.equal(u, v)


def test_captured_forward_replays_the_eager_bits_on_new_contents(net, whole):
    m, _ = net
    x0 = whole[(32, 64)]["x"].to(DEV)
    x1 = torch.from_numpy(RR.syn.rng_normal(99, tuple(x0.shape))).to(DEV)
    with torch.no_grad():
        eager = [[t.clone() for t in m(x)] for x in (x0, x1)]
        torch.cuda.synchronize()
        buf = x0.clone()
        try:
            with fused.scratch_namespace("resnet-capture-test"):
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    m(buf)                                 # (allocates the namespace's scratch outside the capture)
                torch.cuda.current_stream().wait_stream(side)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    captured = m(buf)
            for x, want in ((x1, eager[1]), (x0, eager[0])):
                buf.copy_(x)
                graph.replay()
                torch.cuda.synchronize()
                for c, e in zip(captured, want):
                    assert torch.equal(c, e)
        finally:
            fused.release_scratch("resnet-capture-test")


def test_two_namespaces_do_not_share_scratch(net, whole):
    m, _ = net
    x = whole[(32, 64)]["x"].to(DEV)

    def ptrs(ns):
        return {v.data_ptr() for k, v in fused._conv_images.items() if k[0] == "resnet" and k[-1] == ns}

    try:
        with torch.no_grad():
            for ns in ("resnet-ns-a", "resnet-ns-b"):
                with fused.scratch_namespace(ns):
                    m(x)
        torch.cuda.synchronize()
        a, b = ptrs("resnet-ns-a"), ptrs("resnet-ns-b")
        assert a and b and len(a) == len(b) and not (a & b) and not (a & ptrs(None))
        before = len(fused._conv_images)
        with torch.no_grad(), fused.scratch_namespace("resnet-ns-a"):
            m(x)
        assert len(fused._conv_images) == before        # allocated once per shape
    finally:
        fused.release_scratch("resnet-ns-a")
        fused.release_scratch("resnet-ns-b")
    assert not ptrs("resnet-ns-a")


def test_replacing_a_running_statistic_in_place_repacks(net, whole):
    m, sd = net
    x = whole[(32, 64)]["x"].to(DEV)
    bn = m.layer1[0].bn1
    with torch.no_grad():
        before = [t.clone() for t in m(x)]
        bn.running_mean.add_(0.5)
        try:
            sd2 = dict(sd)
            sd2["layer1.0.bn1.running_mean"] = sd["layer1.0.bn1.running_mean"] + 0.5
            got = m(x)
            assert not torch.equal(got[0], before[0])
            want, fp32 = RR.resnet(sd2, whole[(32, 64)]["x"].double()), RR.resnet(sd2, whole[(32, 64)]["x"])
            within_rule("resnet50 after an in-place running_mean change, stage 0", got[0].cpu(), want[0], fp32[0], stages=STAGES[0],
                        group="repack")
        finally:
            bn.running_mean.copy_(sd["layer1.0.bn1.running_mean"])
        for a, b in zip(m(x), before):
            assert torch.equal(a, b)
