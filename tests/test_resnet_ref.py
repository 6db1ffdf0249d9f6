"""The image backbone without a GPU (racformer_amd/resnet.py): mmdet's keys and shapes, output sizes, the torch route and the input
normalisation against the float64 restatement (tests/resnet_ref.py -- there is no golden from the reference, whose tree has no
ResNet-50: float64 torch is the arbiter), refusals, ``train()``, BatchNorm folding, routing, and the new entry points' declarations
and argument errors."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import resnet_ref as RR
from racformer_amd import ResNet, _lib, resnet
from racformer_amd.radar_pillars import fold_bn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shapes_of(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


@pytest.fixture(scope="module")
def net():
    m = ResNet(50).eval()
    sd = RR.fill_state(shapes_of(m), RR.SEED)
    m.load_state_dict(sd, strict=True)
    return m, sd


def within_rule(what, got, want, fp32, stages=1):
    err = (got.double() - want).abs().max().item()
    e_ref = (fp32.double() - want).abs().max().item()
    wmax = float(want.abs().max())
    print(f"{what}: E_ref={e_ref:.3e} err={err:.3e} max|want|={wmax:.3e}")
    assert err < stages * (max(4 * e_ref, 3e-6 * wmax) + 1e-6), (what, err, e_ref, wmax)


def test_keys_and_shapes_are_mmdets():
    m = ResNet(50)
    assert sorted(m.state_dict()) == RR.expected_keys(50) and len(RR.expected_keys(50)) == 318
    assert shapes_of(m) == RR.expected_shapes(50)
    assert tuple(m.state_dict()["layer3.0.downsample.0.weight"].shape) == (1024, 512, 1, 1)
    assert tuple(m.state_dict()["layer1.0.conv2.weight"].shape) == (64, 64, 3, 3)
    assert tuple(m.state_dict()["conv1.weight"].shape) == (64, 3, 7, 7)
    m.load_state_dict(RR.fill_state(RR.expected_shapes(50), 1), strict=True)
    for depth in (101, 152):
        assert sorted(ResNet(depth).state_dict()) == RR.expected_keys(depth)
    assert sorted(ResNet(50, num_stages=2, out_indices=(0, 1)).state_dict()) == sorted(RR.expected_shapes(50, 2))
    assert ResNet(50).fused is True and ResNet(50).input_norm is None


def test_constructor_names_and_defaults_are_mmdets():
    import inspect
    sig = inspect.signature(ResNet.__init__)
    names = [p for p in sig.parameters if p != "self"]
    assert names == ["depth", "in_channels", "stem_channels", "base_channels", "num_stages", "strides", "dilations", "out_indices",
                     "style", "deep_stem", "avg_down", "frozen_stages", "conv_cfg", "norm_cfg", "norm_eval", "dcn", "stage_with_dcn",
                     "plugins", "with_cp", "zero_init_residual", "pretrained", "init_cfg", "fused"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["in_channels"] == 3 and d["stem_channels"] is None and d["base_channels"] == 64 and d["num_stages"] == 4
    assert d["strides"] == (1, 2, 2, 2) and d["dilations"] == (1, 1, 1, 1) and d["out_indices"] == (0, 1, 2, 3)
    assert d["style"] == 'pytorch' and d["frozen_stages"] == -1 and d["norm_eval"] is True and d["with_cp"] is False
    assert d["norm_cfg"] == dict(type='BN', requires_grad=True) and d["zero_init_residual"] is True and d["fused"] is True


@pytest.mark.parametrize("hw", [(37, 53), (32, 64), (7, 9), (1, 1)])
def test_output_sizes_and_torch_route_vs_float64(net, hw):
    m, sd = net
    x = RR.make_images(hw, norm=False)
    want = RR.resnet(sd, x.double())
    fp32 = RR.resnet(sd, x)
    with torch.no_grad():
        assert not m.hip_route(x)
        got = m(x)
    assert isinstance(got, tuple) and len(got) == 4
    for i, (g, w, f, size) in enumerate(zip(got, want, fp32, RR.stage_sizes(*hw))):
        assert tuple(g.shape) == (x.shape[0], 256 * 2 ** i) + size == tuple(w.shape)
        assert g.is_contiguous() and g.dtype == torch.float32
        within_rule(f"torch route {hw} stage {i}", g, w, f, stages=1)


def test_fixture_stage_maxima_stay_in_range(net):
    """The weight recipe keeps every stage maximum in [1, 1e3]: the fixture cannot drift into overflow or all-zero maps."""
    _, sd = net
    for hw in ((37, 53), (32, 64)):
        for i, w in enumerate(RR.resnet(sd, RR.make_images(hw, norm=False).double())):
            assert 1.0 <= float(w.abs().max()) <= 1.0e3, (hw, i, float(w.abs().max()))


def test_input_norm_matches_the_reference_lines(net):
    m, sd = net
    x = RR.make_images((37, 53), norm=True)
    assert torch.equal(resnet.apply_input_norm(x, RR.NORM), RR.input_norm(x, RR.NORM))
    bgr_only = dict(RR.NORM, to_rgb=False)
    assert torch.equal(resnet.apply_input_norm(x, bgr_only), RR.input_norm(x, bgr_only))
    want = RR.resnet(sd, x.double(), norm=RR.NORM)
    fp32 = RR.resnet(sd, x, norm=RR.NORM)
    m.input_norm = RR.NORM
    try:
        with torch.no_grad():
            got = m(x)
    finally:
        m.input_norm = None
    for i in range(4):
        within_rule(f"torch route with input_norm stage {i}", got[i], want[i], fp32[i])
    with torch.no_grad():
        assert not torch.equal(got[0], m(x)[0])


@pytest.mark.parametrize("kwargs", [dict(depth=18), dict(depth=34), dict(depth=50, style='caffe'), dict(depth=50, deep_stem=True),
                                    dict(depth=50, avg_down=True), dict(depth=50, dcn=dict(type='DCN')),
                                    dict(depth=50, plugins=[dict()]), dict(depth=50, conv_cfg=dict(type='ConvWS')),
                                    dict(depth=50, dilations=(1, 1, 2, 4)), dict(depth=50, norm_cfg=dict(type='GN', num_groups=32)),
                                    dict(depth=50, norm_cfg=dict(type='SyncBN')), dict(depth=50, in_channels=4)])
def test_unused_options_are_refused(kwargs):
    with pytest.raises(NotImplementedError):
        ResNet(**kwargs)


def test_accepted_options():
    for kwargs in (dict(depth=101), dict(depth=152), dict(depth=50, num_stages=1, out_indices=(0,)), dict(depth=50, with_cp=True),
                   dict(depth=50, norm_cfg=dict(type='BN2d', requires_grad=False)), dict(depth=50, fused=False)):
        ResNet(**kwargs)
    with pytest.raises(KeyError):
        ResNet(51)


def bns(m):
    return [b for b in m.modules() if isinstance(b, nn.modules.batchnorm._BatchNorm)]


def test_train_keeps_batchnorms_in_eval_and_freezes_stages():
    m = ResNet(50, norm_eval=True)
    m.train()
    assert m.training and all(not b.training for b in bns(m)) and len(bns(m)) == 53
    assert all(p.requires_grad for p in m.parameters())
    m = ResNet(50, frozen_stages=1, norm_eval=False)
    m.train()
    frozen = list(m.conv1.parameters()) + list(m.bn1.parameters()) + list(m.layer1.parameters())
    assert all(not p.requires_grad for p in frozen) and not m.bn1.training and not m.layer1.training
    assert all(not b.training for b in bns(m.layer1)) and all(b.training for b in bns(m.layer2))
    assert all(p.requires_grad for p in m.layer2.parameters()) and m.layer2.training
    x = torch.zeros(1, 3, 8, 8)
    with torch.no_grad():
        assert not m.hip_route(x)                # norm_eval=False in training: batch statistics, the torch route
    m = ResNet(50, norm_cfg=dict(type='BN', requires_grad=False))
    assert all(not p.requires_grad for b in bns(m) for p in b.parameters()) and m.conv1.weight.requires_grad


def test_folding_reproduces_bn_of_conv_in_float64(net):
    m, _ = net
    x = torch.from_numpy(RR.syn.rng_normal(3, (2, 64, 5, 6))).double()
    for conv, bn, kw in ((m.layer1[0].conv2, m.layer1[0].bn2, dict(padding=1)), (m.layer1[0].downsample[0], m.layer1[0].downsample[1], {}),
                         (m.layer1[0].conv1, m.layer1[0].bn1, {})):
        w, shift = fold_bn(conv.weight, bn)
        want = F.batch_norm(F.conv2d(x, conv.weight.detach().double(), None, **kw), bn.running_mean.double(), bn.running_var.double(),
                            bn.weight.detach().double(), bn.bias.detach().double(), training=False, eps=bn.eps)
        got = F.conv2d(x, w.double(), shift.double(), **kw)
        # the folded operands are float32: one rounding of each weight and shift
        assert (got - want).abs().max().item() < 4e-7 * float(want.abs().max()) * 4
    assert tuple(resnet.pack_stem_weight(fold_bn(m.conv1.weight, m.bn1)[0]).shape) == (147, 64)
    w, _ = fold_bn(m.conv1.weight, m.bn1)
    assert torch.equal(resnet.pack_stem_weight(w)[(1 * 7 + 2) * 7 + 3], w[:, 1, 2, 3])


def test_cpu_tensors_never_take_the_hip_route(net):
    m, _ = net
    x = torch.zeros(1, 3, 8, 8)
    with torch.no_grad():
        assert not m.hip_route(x) and not m.hip_route(x.double())
    assert not m.hip_route(x)
    # the launcher's tile rule at the f8 shapes (48 images) and online (6): wide tiles while every CU still gets a workgroup
    assert resnet.conv_tile_channels(256, 48, 64, 176) == (256, 8448) and resnet.conv_tile_channels(64, 48, 64, 176) == (64, 8448)
    assert resnet.conv_tile_channels(2048, 48, 8, 22) == (256, 1152) and resnet.conv_tile_channels(512, 48, 8, 22) == (256, 288)
    assert resnet.conv_tile_channels(2048, 6, 8, 22) == (128, 288) and resnet.conv_tile_channels(512, 6, 8, 22) == (64, 144)
    assert resnet.conv_tile_channels(384, 48, 64, 176) == (128, 3 * 8448)
    assert resnet.stem_sizes(256, 704) == ((128, 352), (64, 176)) and resnet.stem_sizes(1, 1) == ((1, 1), (1, 1))


# ----------------------------------------------------------------------------------------------------------------------- ABI
def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "racformer_hip.h")).read(), flags=re.S)
    want = {"rac_resnet_stem_fwd": "pp", "rac_resnet_absmax_fwd": "ppilp", "rac_resnet_conv_fwd": "pp"}
    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_float: "f", ctypes.c_int64: "l"}
    for name, kinds in want.items():
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert "".join(kind[a] for a in _lib.SIGNATURES[name][1]) == kinds
        assert hasattr(_lib.lib(), name)
    assert int(re.search(r"#define\s+RAC_ABI_VERSION\s+(\d+)", text).group(1)) >= 28


def conv_desc(**over):
    one = ctypes.c_void_p(64)
    f = dict(in_=one, w_image=one, bias=one, residual=None, amax_parts=one, out=one, w_alpha=1.0, N=1, H=4, W=4, Cin=64, Cout=64,
             ksize=3, stride=1, relu=1)
    f.update(over)
    return _lib.ResnetConv(**f)


@pytest.mark.parametrize("over,msg", [(dict(in_=None), b"null pointer"), (dict(w_image=None), b"null pointer"),
                                      (dict(out=None), b"null pointer"), (dict(amax_parts=None), b"null pointer"),
                                      (dict(Cin=48), b"Cin=48"), (dict(Cin=0), b"Cin=0"), (dict(Cin=4096), b"Cin=4096"),
                                      (dict(Cout=96), b"Cout=96"), (dict(Cout=32), b"Cout=32"), (dict(ksize=5), b"ksize=5"),
                                      (dict(ksize=2), b"ksize=2"), (dict(stride=3), b"stride=3"), (dict(stride=0), b"stride=0"),
                                      (dict(H=0), b"must be positive"), (dict(W=-1), b"must be positive"),
                                      (dict(N=0), b"must be positive")])
def test_conv_argument_errors_need_no_gpu(over, msg):
    lib = _lib.lib()
    rc = lib.rac_resnet_conv_fwd(ctypes.byref(conv_desc(**over)), None)
    assert rc == -1 and msg in lib.rac_last_error(), lib.rac_last_error()


def test_stem_and_absmax_argument_errors_need_no_gpu():
    lib = _lib.lib()
    assert lib.rac_resnet_conv_fwd(None, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_resnet_stem_fwd(None, None) == -1 and b"null pointer" in lib.rac_last_error()
    one = ctypes.c_void_p(64)
    ok = dict(img=one, w=one, bias=one, conv=one, out=one, N=1, H=8, W=8, norm=0)
    for over, msg in ((dict(img=None), b"null pointer"), (dict(conv=None), b"null pointer"), (dict(H=0), b"must be positive"),
                      (dict(N=0), b"must be positive"), (dict(w=ctypes.c_void_p(68)), b"16-byte aligned")):
        d = _lib.ResnetStem(**dict(ok, **over))
        assert lib.rac_resnet_stem_fwd(ctypes.byref(d), None) == -1 and msg in lib.rac_last_error(), lib.rac_last_error()
    d = _lib.ResnetStem(**dict(ok, norm=1))
    d.perm[0] = 3
    assert lib.rac_resnet_stem_fwd(ctypes.byref(d), None) == -1 and b"perm[0]=3" in lib.rac_last_error()
    assert lib.rac_resnet_absmax_fwd(None, one, 1, 8, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_resnet_absmax_fwd(one, one, 0, 8, None) == -1 and b"N=0" in lib.rac_last_error()
    assert lib.rac_resnet_absmax_fwd(one, one, 1, 0, None) == -1 and b"per_image=0" in lib.rac_last_error()
