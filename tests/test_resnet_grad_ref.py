"""The image backbone's backward without a GPU (racformer_amd/resnet.py ``fused_grad``, csrc/resnet_bwd.hip): the fold backward
against float64 autograd, the new entry points' declarations and argument errors, the switch and the routing on CPU tensors, the
weight gradient's K-range rule."""
import ctypes
import inspect
import os
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import resnet_ref as RR
from racformer_amd import ResNet, _lib, resnet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------------------------- fold backward
def _conv_bn(cin, cout, k, seed):
    conv, bn = nn.Conv2d(cin, cout, k, padding=k // 2, bias=False), nn.BatchNorm2d(cout).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(RR.syn.rng_normal(seed, (cout, cin, k, k), 0.2)))
        bn.weight.copy_(torch.from_numpy(RR.syn.rng_uniform(seed + 1, (cout,), 0.5, 1.5)))
        bn.bias.copy_(torch.from_numpy(RR.syn.rng_normal(seed + 2, (cout,), 0.3)))
        bn.running_mean.copy_(torch.from_numpy(RR.syn.rng_normal(seed + 3, (cout,), 0.7)))
        bn.running_var.copy_(torch.from_numpy(RR.syn.rng_uniform(seed + 4, (cout,), 0.3, 2.5)))
    return conv, bn


def _fold64(w, gamma, beta, mean, var, eps):
    s = gamma / torch.sqrt(var + eps)
    return w * s.view(-1, 1, 1, 1), beta - mean * s


@pytest.mark.parametrize("k", [1, 3])
def test_fold_bn_backward_against_float64_autograd(k):
    """(a) all three gradients: within 1e-6 of the largest element (one float32 rounding of the result)"""
    conv, bn = _conv_bn(6, 8, k, 7100 + k)
    dwf = torch.from_numpy(RR.syn.rng_normal(7200 + k, (8, 6, k, k)))
    dbf = torch.from_numpy(RR.syn.rng_normal(7300 + k, (8,)))
    w, g, b = (t.detach().double().clone().requires_grad_() for t in (conv.weight, bn.weight, bn.bias))
    wf, sh = _fold64(w, g, b, bn.running_mean.double(), bn.running_var.double(), bn.eps)
    ((wf * dwf.double()).sum() + (sh * dbf.double()).sum()).backward()
    got = resnet.fold_bn_backward(dwf, dbf, conv.weight, bn)
    for name, have, want in zip(("dW", "dgamma", "dbeta"), got, (w.grad, g.grad, b.grad)):
        assert have.dtype == torch.float32 and have.shape == want.shape
        err, big = float((have.double() - want).abs().max()), float(want.abs().max())
        print(f"fold backward k={k} {name}: err {err:.3e} of {big:.3e}")
        assert err <= 1e-6 * big, (name, err, big)
    # the forward it mirrors: folding and convolving is BatchNorm of the convolution
    x = torch.from_numpy(RR.syn.rng_normal(7400, (2, 6, 5, 4))).double()
    want = F.batch_norm(F.conv2d(x, w.detach(), None, padding=k // 2), bn.running_mean.double(), bn.running_var.double(), g.detach(),
                        b.detach(), training=False, eps=bn.eps)
    assert float((F.conv2d(x, wf.detach(), sh.detach(), padding=k // 2) - want).abs().max()) < 1e-12


def test_fold_bn_backward_computes_only_what_is_required():
    """(b) gradients that are not required are None, the others unchanged"""
    conv, bn = _conv_bn(6, 8, 3, 7500)
    dwf = torch.from_numpy(RR.syn.rng_normal(7600, (8, 6, 3, 3)))
    dbf = torch.from_numpy(RR.syn.rng_normal(7700, (8,)))
    full = resnet.fold_bn_backward(dwf, dbf, conv.weight, bn)
    bn.weight.requires_grad_(False)
    bn.bias.requires_grad_(False)
    dw, dg, db = resnet.fold_bn_backward(dwf, None, conv.weight, bn)
    assert dg is None and db is None and torch.equal(dw, full[0])
    conv.weight.requires_grad_(False)
    bn.weight.requires_grad_(True)
    dw, dg, db = resnet.fold_bn_backward(dwf, dbf, conv.weight, bn)
    assert dw is None and db is None and torch.equal(dg, full[1])
    dw, dg, db = resnet.fold_bn_backward(dwf, dbf, conv.weight, bn, need=(False, False, True))
    assert dw is None and dg is None and torch.equal(db, full[2]) and torch.equal(db, dbf)


# ----------------------------------------------------------------------------------------------------------------------- ABI
def test_new_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "racformer_hip.h")).read(), flags=re.S)
    want = {"rac_resnet_conv_dgrad": "pp", "rac_resnet_conv_wgrad": "ppppp" + "i" * 10 + "p", "rac_resnet_relu_bwd": "pppplp"}
    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_float: "f", ctypes.c_int64: "l"}
    for name, kinds in want.items():
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert "".join(kind[a] for a in _lib.SIGNATURES[name][1]) == kinds
        assert hasattr(_lib.lib(), name)
    assert int(re.search(r"#define\s+RAC_ABI_VERSION\s+(\d+)", text).group(1)) >= 30
    assert _lib.lib().rac_abi_version() >= 30
    fields = [n for n, _ in _lib.ResnetDgrad._fields_]
    struct = re.search(r"typedef struct \{([^}]*)\}\s*rac_resnet_dgrad;", text).group(1)
    assert fields == re.findall(r"(\w+)\s*[;,]", struct)


def dgrad_desc(**over):
    one = ctypes.c_void_p(64)
    f = dict(g=one, w_image=one, add=None, mask=None, amax_parts=one, out=one, w_alpha=1.0, N=1, H=4, W=4, Ho=4, Wo=4, Cin=64, Cout=64,
             ksize=3, stride=1)
    f.update(over)
    return _lib.ResnetDgrad(**f)


@pytest.mark.parametrize("over,msg", [(dict(g=None), b"null pointer"), (dict(w_image=None), b"null pointer"),
                                      (dict(out=None), b"null pointer"), (dict(amax_parts=None), b"null pointer"),
                                      (dict(Cin=96), b"Cin=96"), (dict(Cin=32), b"Cin=32"), (dict(Cin=0), b"Cin=0"),
                                      (dict(Cin=4096), b"Cin=4096"), (dict(Cout=48), b"Cout=48"), (dict(Cout=0), b"Cout=0"),
                                      (dict(Cout=4096), b"Cout=4096"), (dict(ksize=5), b"ksize=5"), (dict(ksize=2), b"ksize=2"),
                                      (dict(stride=3), b"stride=3"), (dict(stride=0), b"stride=0"), (dict(H=0), b"must be positive"),
                                      (dict(W=-1), b"must be positive"), (dict(N=0), b"must be positive"),
                                      (dict(Ho=0), b"does not map"), (dict(Ho=3), b"does not map"), (dict(Wo=5), b"does not map"),
                                      (dict(stride=2), b"does not map"), (dict(stride=2, H=9, W=8, Ho=4, Wo=4), b"does not map"),
                                      (dict(w_image=ctypes.c_void_p(72)), b"16-byte aligned")])
def test_dgrad_argument_errors_need_no_gpu(over, msg):
    lib = _lib.lib()
    rc = lib.rac_resnet_conv_dgrad(ctypes.byref(dgrad_desc(**over)), None)
    assert rc == -1 and msg in lib.rac_last_error(), lib.rac_last_error()


def wgrad_args(**over):
    one = ctypes.c_void_p(64)
    f = dict(g=one, x=one, workspace=one, dw=one, db=one, N=2, Cin=64, H=7, W=8, Cout=64, Ho=4, Wo=4, ksize=3, stride=2, k_splits=2)
    f.update(over)
    return [f[k] for k in ("g", "x", "workspace", "dw", "db", "N", "Cin", "H", "W", "Cout", "Ho", "Wo", "ksize", "stride", "k_splits")]


@pytest.mark.parametrize("over,msg", [(dict(g=None), b"null pointer"), (dict(x=None), b"null pointer"),
                                      (dict(workspace=None), b"null pointer"), (dict(dw=None), b"null pointer"),
                                      (dict(Cin=48), b"Cin=48"), (dict(Cin=0), b"Cin=0"), (dict(Cin=4096), b"Cin=4096"),
                                      (dict(Cout=96), b"Cout=96"), (dict(Cout=32), b"Cout=32"), (dict(Cout=4096), b"Cout=4096"),
                                      (dict(ksize=5), b"ksize=5"), (dict(ksize=2), b"ksize=2"), (dict(stride=3), b"stride=3"),
                                      (dict(stride=0), b"stride=0"), (dict(H=0), b"must be positive"), (dict(W=-1), b"must be positive"),
                                      (dict(N=0), b"must be positive"), (dict(Ho=0), b"does not map"), (dict(Ho=3), b"does not map"),
                                      (dict(H=9), b"does not map"), (dict(stride=1), b"does not map"),
                                      (dict(k_splits=0), b"k_splits=0"), (dict(k_splits=3), b"k_splits=3"),
                                      (dict(N=5, k_splits=4), b"empty range")])
def test_wgrad_argument_errors_need_no_gpu(over, msg):
    """(2 images of 4 x 4 output pixels are 2 K units; 5 units in 4 ranges of 2 leave the last one empty)"""
    lib = _lib.lib()
    rc = lib.rac_resnet_conv_wgrad(*wgrad_args(**over), None)
    assert rc == -1 and msg in lib.rac_last_error(), lib.rac_last_error()


def test_null_descriptor_and_relu_bwd_argument_errors_need_no_gpu():
    lib = _lib.lib()
    one = ctypes.c_void_p(64)
    assert lib.rac_resnet_conv_dgrad(None, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_resnet_relu_bwd(None, one, None, one, 8, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_resnet_relu_bwd(one, one, None, None, 8, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_resnet_relu_bwd(one, one, None, one, 0, None) == -1 and b"count=0" in lib.rac_last_error()


# ----------------------------------------------------------------------------------------------------------- switch and routing
def test_the_switch_is_a_class_attribute_and_off():
    assert ResNet.fused_grad is False and ResNet(50).fused_grad is False
    assert "fused_grad" not in inspect.signature(ResNet.__init__).parameters
    names = [p for p in inspect.signature(ResNet.__init__).parameters if p != "self"]
    assert names[0] == "depth" and names[-1] == "fused" and len(names) == 23


def test_cpu_tensors_take_the_torch_route_with_the_switch_on():
    m = ResNet(50, frozen_stages=1)
    m.load_state_dict(RR.fill_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, RR.SEED))
    m.train()
    m.fused_grad = True
    x = RR.make_images((7, 9), norm=False)
    assert not m.hip_grad_route(x) and not m.hip_route(x)
    outs = m(x)
    assert [o.requires_grad for o in outs] == [False, True, True, True]      # (layer1 is frozen)
    sum(o.sum() for o in outs).backward()
    assert m.layer2[0].conv1.weight.grad is not None and m.layer1[0].conv1.weight.grad is None and m.conv1.weight.grad is None
    with torch.no_grad():
        assert not m.hip_grad_route(x)
    assert resnet.trainable_blocks(m) == [(i, b) for i, nb in ((1, 4), (2, 6), (3, 3)) for b in range(nb)]
    assert resnet.trainable_blocks(ResNet(50, frozen_stages=4)) == []


def test_conv_wgrad_k_splits_is_a_function_of_the_shape():
    ks = resnet.conv_wgrad_k_splits
    # f8 shapes (48 images), tiles of 128 x 128: layer2 3x3, layer4 3x3 (144 tiles), layer2.0 conv3, layer4 conv3
    assert ks(48, 32, 88, 128, 128, 3) == 56 and ks(48, 8, 22, 512, 512, 3) == 3
    assert ks(48, 32, 88, 128, 512, 1) == 128 and ks(48, 8, 22, 512, 2048, 1) == 8
    # never more ranges than K units, none empty
    assert ks(1, 1, 1, 64, 64, 1) == 1 and ks(2, 4, 6, 64, 64, 1) == 2 and ks(2, 4, 6, 32, 64, 3) == 2
    for n, ho, wo, cin, cout, k in ((3, 16, 44, 64, 64, 3), (6, 64, 176, 64, 64, 3), (2, 7, 11, 2048, 512, 1), (5, 3, 3, 96, 128, 1)):
        units, got = n * ((ho * wo + 31) // 32), ks(n, ho, wo, cin, cout, k)
        per = -(-units // got)
        assert 1 <= got <= units and (got - 1) * per < units
    assert ks(6, 64, 176, 64, 64, 3) > 50
