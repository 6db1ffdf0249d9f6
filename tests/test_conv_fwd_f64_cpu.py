"""tests/conv_fwd_ref.py on the CPU: every check of tests/test_conv_fwd_f64_gpu.py with the float32 restatements in the kernels'
place -- the proof, made without a device, that the cases leave the float32 arithmetic inside the bound, that the references and
the restated launcher rules reach every instantiation and path -- and each negative control failing its check."""
import ctypes

import pytest
import torch

import conv_fwd_ref as V
from racformer_amd import _lib

CD_MODES = {"image": _lib.CD_IMAGE, "f32": _lib.CD_F32, "gru": _lib.CD_GRU, "image_relu": _lib.CD_IMAGE_RELU, "f32_cf_relu": _lib.CD_F32_CF_RELU}

RUN = V.Restated()


@pytest.fixture(scope="module")
def log():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    lg = V.Log()
    yield lg
    torch.set_num_threads(n)


def test_absmax():
    assert V.check_absmax(RUN) == {"deep", "single", "tail"}


@pytest.mark.parametrize("W", V.PACK_WIDTHS)
@pytest.mark.parametrize("kind", V.PACK_KINDS)
def test_pack(kind, W):
    path = V.check_pack(RUN, kind, W)
    assert path == (("vector" if W in (4, 128) else "scalar"), {1: 1, 3: 1, 4: 1, 17: 1, 128: 1, 130: 2, 257: 3}[W])


@pytest.mark.parametrize("magnitude", ["tiny", "zero"])
@pytest.mark.parametrize("kind,W", [("nchw", 17), ("nchw", 128), ("cl", 17), ("live1", 4), ("live4", 130)])
def test_pack_magnitudes(kind, W, magnitude):
    V.check_pack(RUN, kind, W, magnitude)


@pytest.mark.parametrize("name", V.CONV_PLAIN)
def test_conv3x3(log, name):
    V.check_conv(log, name, RUN)


@pytest.mark.parametrize("name", V.CONV_POISON)
def test_conv3x3_poisoned(log, name):
    V.check_conv_poison(log, name, RUN)


@pytest.mark.parametrize("name", list(V.TEMPORAL_CASES))
def test_temporal(log, name):
    V.check_temporal(log, name, RUN)


@pytest.mark.parametrize("name", list(V.S2_CASES))
def test_conv3x3s2(log, name):
    V.check_s2(log, name, RUN)


@pytest.mark.parametrize("name", V.DIRECT_PLAIN + V.DIRECT_POISON)
def test_conv_direct(log, name):
    V.check_direct(log, name, RUN)


@pytest.mark.parametrize("name", list(V.UPSAMPLE_CASES))
def test_upsample_image(log, name):
    V.check_upsample(log, name, RUN)


def test_everything_was_reached(log):
    """(after the cases above) every output mode, tile shape, chunk count and all eleven instantiations of conv_direct_kernel"""
    assert len(V.CD_INSTANCES) == 11
    assert V.REACH <= log.reached, sorted(V.REACH - log.reached)
    assert all(e["ratio"] <= 1.0 for e in log.errors.values())


def test_launcher_rules():
    """the restated dispatch refuses what rac_conv_direct_fwd refuses, and the tile rules at the issue's maps"""
    assert V.cd_instance("gru", 1, 1) is None and V.cd_instance("image", 2, 4) is None and V.cd_instance("image_relu", 2, 2) is None
    assert V.cd_instance("image", 1, 3) is None and V.cd_instance("f32", 1, 3) is None and V.cd_instance("f32_cf_relu", 1, 1) is None
    assert {V.cd_instance(m, s, k)[0] for m, s, k in (("gru", 1, 0), ("gru", 1, 2), ("image", 2, 2), ("image", 2, 3), ("image", 2, 8), ("image", 1, 2),
                                                      ("image_relu", 1, 2), ("f32", 1, 1), ("f32", 1, 2), ("f32", 1, 4), ("f32_cf_relu", 1, 2))} \
        == set(V.CD_INSTANCES)
    assert [V.conv_tiles(H, W) for H, W in V.MAPS] == [(1, 1), (1, 15), (1, 256), (2, 16), (2, 5), (2, 4), (2, 256)]
    assert V.absmax_paths(V.ABSMAX_BIG) == dict(deep=True, single=True, tail=True)
    assert V.absmax_paths(1024) == dict(deep=False, single=True, tail=False) and V.absmax_paths(3) == dict(deep=False, single=False, tail=True)


@pytest.mark.parametrize("fault", V.FAULTS)
def test_negative_control_fails(fault):
    """each deliberately wrong restatement misses its check; the same check passes without the fault (the tests above)"""
    check, name = V.FAULT_CASES[fault]
    with pytest.raises(V.OutOfBound):
        V.CHECKS[check](V.Log(), name, V.Restated(fault))


def test_host_forms():
    assert V.act_scale(0.0) == 1.0 and V.act_scale(float("inf")) == 1.0 and V.act_scale(float("nan")) == 1.0 and V.act_scale(1e-31) == 1.0
    assert V.act_scale(1.0) == 2.0 ** 13 and V.act_scale(0.99) == 2.0 ** 14 and V.act_scale(6.0) == 2.0 ** 11
    q, s = V.quantize_host(torch.tensor([[1.0] + [0.0] * 63, [float("nan")] + [3.0] * 63, [0.0] * 64]))
    assert q[0, 0] == 2 ** 14 and float(s[0]) == 2.0 ** -14 and bool(torch.isnan(s[1])) and int(q[1, 0]) == -32767 and int(q[1, 1]) == 0
    assert int(q[2].abs().max()) == 0 and float(s[2]) == 2.0 ** (15 - 141)


def test_refusals():
    """what the restated dispatch calls refused, rac_conv_direct_fwd refuses (no launch)"""
    d = _lib.ConvDirect()
    p = ctypes.c_void_p(256)
    d.N, d.H, d.W, d.in_img, d.ws, d.in_chunks_total, d.Cout, d.out_img, d.out_f32, d.out_chunks_total = 1, 4, 4, p, p, 8, 64, p, p, 8
    for fr in ("in_frames", "out_frames", "xpart_frames", "h_prev_frames", "h_out_frames"):
        setattr(d, fr, _lib.CdFrames(1, 1, 0))
    for mode, stride, k in (("image", 2, 4), ("image_relu", 2, 2), ("image", 1, 3), ("f32", 1, 3), ("f32_cf_relu", 1, 1)):
        assert V.cd_instance(mode, stride, k) is None
        d.mode, d.conv_stride, d.chunks = CD_MODES[mode], stride, k
        assert _lib.lib().rac_conv_direct_fwd(ctypes.byref(d), None) == -1, (mode, stride, k)
