"""tests/depth_net_fwd_ref.py on the CPU: every check of tests/test_depth_net_fwd_f64_gpu.py with the float32 restatement in the
kernels' place -- the proof, made without a device, that the cases leave float32 arithmetic in the kernels' order inside the bound
and that the references and the restated launcher rules reach every path -- and each negative control failing its check."""
import ctypes

import pytest
import torch

import depth_net_fwd_ref as V
from racformer_amd import _lib

RUN = V.Restated()


@pytest.fixture(scope="module")
def log():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    lg = V.Log()
    yield lg
    torch.set_num_threads(n)


@pytest.mark.parametrize("name", list(V.PACK_CASES))
def test_pack(name):
    V.check_pack(RUN, name)


def test_pack_of_no_image_writes_nothing():
    V.check_pack(RUN, "C33 hw33", BN0=True)


@pytest.mark.parametrize("name", V.CONV_PLAIN)
def test_conv_small(log, name):
    V.check_conv(log, name, RUN)


@pytest.mark.parametrize("name", V.CONV_POISON)
def test_conv_small_poisoned(log, name):
    V.check_conv(log, name, RUN)


def test_conv_small_of_no_image_writes_nothing():
    V.check_conv_bn0(RUN)


@pytest.mark.parametrize("name", list(V.GATES_CASES))
def test_gates(log, name):
    V.check_gates(log, name, RUN)


@pytest.mark.parametrize("name", list(V.POOL_CASES))
def test_pool_bias(log, name):
    V.check_pool(log, name, RUN)


def test_everything_was_reached(log):
    """(after the cases above) every tile shape, tap set, chunk count, channel-tile class, epilogue part, layout, gating and G"""
    assert V.REACH <= log.reached, sorted(V.REACH - log.reached)
    assert all(e["ratio"] <= 1.0 for e in log.errors.values())


def test_launcher_rules():
    """the rules restated at the issue's shapes"""
    assert [V.conv_tiles(H, W) for H, W in ((1, 1), (3, 5), (8, 8), (7, 11), (16, 44), (20, 23))] == [(1, 1), (1, 15), (1, 64), (2, 13), (11, 64), (8, 12)]
    assert V.live_taps(1, 1, 3, 1) == (4,) and V.live_taps(8, 5, 3, 6) == (1, 4, 7) and V.live_taps(5, 8, 3, 6) == (3, 4, 5)
    assert V.live_taps(16, 44, 3, 18) == (3, 4, 5) and V.live_taps(16, 44, 3, 12) == tuple(range(9)) and V.live_taps(20, 23, 3, 18) == tuple(range(9))
    assert V.live_taps(6, 7, 3, 6) == (3, 4, 5) and V.live_taps(6, 7, 3, 6, fault="dead_tap_le") == tuple(range(9))
    assert V.live_taps(3, 5, 1, 1) == (0,)
    assert [V.pool_segments(704, C)[0] for C in (1, 96, 256, 300, 1024)] == [1024, 10, 4, 3, 1]
    assert V.pool_segments(3, 96)[1] == [(0, 0), (0, 0), (0, 0), (0, 1), (1, 1), (1, 1), (1, 2), (2, 2), (2, 2), (2, 3)]
    assert len({V.cout_class(k) for k in (1, 24, 33, 64, 96, 256)}) == 6


@pytest.mark.parametrize("fault", V.FAULTS)
def test_negative_control_fails(fault):
    """each deliberately wrong restatement misses its check; the same check passes without the fault (the tests above)"""
    check, name = V.FAULT_CASES[fault]
    with pytest.raises(V.OutOfBound):
        V.CHECKS[check](V.Log(), name, V.Restated(fault))


def test_chained_k_steps_stay_inside_the_bound():
    """the partial sums of a K step chained on instead of restarted: a change of rounding alone.  It fails no check (measured here:
    kernel figure 3.41 x 2^-24 A against 0.73 restarted on 256 channels x 9 taps, allowed 13.7 -- torch's float32 conv2d on the CPU
    is that very 2304-term chain, E_ref 3.41), so it is no negative control: it runs here to keep the figure, and is not expected to
    fail"""
    lg = V.Log()
    V.check_conv(lg, "8x8 d1 256->256", V.Restated("k_step_chained"))
    V.check_conv(lg, "8x8 one image x 2^-12", V.Restated("k_step_chained"))


def test_refusals():
    """what the header calls a violation is RAC_E_ARG before any launch (no GPU is touched: every call returns at an argument check)"""
    L, p = _lib.lib(), ctypes.c_void_p(256)
    d = _lib.ConvSmall()
    d.in_, d.w, d.out = p, p, p
    d.BN, d.H, d.W, d.Cin, d.Cout, d.ksize, d.dilation, d.ld_in, d.ld_w, d.ld_out = 1, 4, 4, 32, 33, 3, 1, 32, 64, 33
    for field, bad in (("Cin", 48), ("Cin", 0), ("ld_in", 28), ("ld_in", 34), ("ld_w", 32), ("ld_w", 96 + 4), ("Cout", 0), ("ksize", 2), ("dilation", 0),
                       ("ld_out", 32), ("c_off", 1), ("out_layout", 2), ("H", 0)):
        good = getattr(d, field)
        setattr(d, field, bad)
        assert L.rac_conv_small_fwd(ctypes.byref(d), None) == -1, (field, bad)
        setattr(d, field, good)
    d.gate, d.gate_channels = p, 64                       # more gated channels than Cin
    assert L.rac_conv_small_fwd(ctypes.byref(d), None) == -1
    d.gate, d.gate_channels, d.residual, d.ld_res = None, 0, p, 32
    assert L.rac_conv_small_fwd(ctypes.byref(d), None) == -1
    assert L.rac_conv_small_pack_fwd(p, p, 1, 5, 4, 8, 2, 2, None) == -1          # channels 2..8 do not fit rows of 8
    assert L.rac_depthnet_gates_fwd(p, p, p, 1, 1025, 1, None) == -1 and L.rac_depthnet_gates_fwd(p, p, p, 1, 0, 1, None) == -1
    assert L.rac_depthnet_pool_bias_fwd(p, p, p, p, p, 1, 4, 1024, 1025, 1, None) == -1
    assert L.rac_depthnet_pool_bias_fwd(p, p, p, p, p, 1, 4, 95, 96, 1, None) == -1
