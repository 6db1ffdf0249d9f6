"""DepthNet's forward kernels on the MI355X against float64, element by element: cs_pack_kernel, cs_conv_kernel, dn_gates_kernel and
dn_pool_bias_kernel (csrc/depth_net.hip).  tests/depth_net_fwd_ref.py holds the cases, the references, the magnitudes, the
restatement, the negative controls and the launchers' rules restated; tests/test_depth_net_fwd_f64_cpu.py runs the same checks on
the CPU with the restatement in the kernels' place and shows that each of the eighteen negative controls fails its check.

Through racformer_amd.depth_net.conv_small and pack_rows, and the C ABI for the two vector kernels (and for the BN = 0 launches: an
empty tensor has no address to hand to the wrappers).

Stage A: every word of the rows cs_pack_kernel writes equals the restatement's -- the source's bits (a -0.0, a NaN, a subnormal) in
channels c_off .. c_off + C - 1, +0 in the c_pad channels behind, the sentinel elsewhere -- at C in {1, 25, 31, 32, 33, 129}, hw in
{1, 31, 32, 33, 77, 704}, BN in {1, 3}, c_off in {0, 256, 281}, c_pad in {0, 7}, the module's own 313 -> 320 among them.
Stage B, per element: |got - ref| <= max(4 x E_ref, 1) x 2^-24 x A; A == 0 means exactly 0; NaN exactly where float64 has NaN; the
rest of every destination (frames before and behind, channels beside c_off .. c_off + Cout - 1, both layouts) still NaN; the unread
input channels NaN, the unread weight columns 3e30.  Stage C: the gates with max(4 x E_ref, 1) x 2^-24 x A_s / 4 + 2^-22 |ref|, the
pool bias with the stage B rule.  Reached, asserted by test_everything_was_reached from the rules restated in the helper: one and
more tiles, whole and ragged last tiles, the tap sets 1x1 / centre only / a column of taps / a row of taps / all nine, 1 / 3 / 8 /
32 chunks, Cout 1 / 24 / 33 / 64 / 96 / 256, every epilogue part alone and all together, both layouts, gates on all and on some
channels, G in {1024, 10, 4, 3, 1} with empty segments and idle threads, the c += 256 loop of the gates.

Measured on the MI355X (83 tests in 2.5 s; profiles/depth_net_fwd_f64.json, written with RAC_DEPTH_NET_FWD_ERRORS=<file>), worst over
the session in units of 2^-24 x A (E_ref | kernel) and the largest err over what the criterion allows:
  conv_small channel-last    6.09 | 3.89   0.43   (the worst ratio on 6 x 7 at dilation 6: E_ref 1.45, kernel 2.47)
  conv_small channel-first   4.03 | 2.40   0.25
  gates                      1.06 | 1.06   0.07   (C = 1, where every route is the same three products; C >= 256: 0.002 | 0.003 -- the
                                                   magnitude carried through three layers of |W| is far above what the sums lose)
  pool_bias                  0.12 | 0.12   0.12
Over the 56 convolution pairs the median is 2.8 | 1.6: the restart every 32 channels keeps the kernel under torch's own float32
convolution, and in most cases with Cin = 32 and three taps or fewer the two have the same worst figure.  The image x 2^-12
(2.9 | 0.5 and 2.5 | 1.9 on its own elements), the 24-channel heads, the dead-tap maps and the poisoned launches are no worse than
their neighbours.  Power-of-two invariance (k = 20, -30), the all-zero input and the all-zero weight giving the epilogue's constants,
the saturated sigmoids (exactly 0 and 1, as float64 rounded to float32) and every word of the pack's destination: bit for bit.
Nothing was written outside a destination.

Found by this module and fixed with it: the four ReLUs of depth_net.hip (cs_conv_kernel's epilogue, both ReLUs of dn_gates_kernel,
dn_pool_bias_kernel's) were fmaxf(v, 0.f), which returns 0 for a NaN.  Before, on the parent's kernels, 11 of the 83 tests failed,
each with "NaN in 0 elements where float64 has none, none in N where it has": the seven poisoned convolutions with relu (N = 297:
nine taps x 33 channels at dilation 6; 72: three live taps x 24 channels at dilation 18; 2541 for a NaN gate: that image; 1 residual
element; 77: one img_bias channel of that image; 1221 and 3 for a NaN row of the bins / cls table), "C257 poison" and "C9 poison" of
the gates (771 and 9: the poisoned image's gates in every branch came out finite) and both poisoned pool biases (256 and 1100).  The
same cases without relu passed.  After (rac_relu): all 83 pass; every finite result keeps its bits -- tests/test_depth_net_gpu.py,
the LSS and the detector tests untouched and green.  Of the issue's negative controls two cannot fail a check of values and are
handled as tests/depth_net_fwd_ref.py says: the dead-tap test with <= (a tap that reads padding alone adds an exact zero; caught in
the rule restated) and the K steps chained on (rounding alone; measured in the CPU module).
The pillar maximum of radar_pillars.hip had the same defect (fmaxf dropped a NaN point feature):
tests/test_radar_pillars_gpu.py::test_2b_nan_point_feature_poisons_its_pillar_alone failed on the parent's kernels in both cases (the
poisoned pillar's 64 channels finite) and passes now.
tools/kernel_isa.py: of the 40 sources only depth_net.hip's and radar_pillars.hip's device assembly changed.
Cost of the fixes, the parent's and the fixed library taking turns on one machine, three runs each, medians in us.
tools/depth_net_bench.py (f8 shape, 100 repetitions): the step of 6 maps eager 1339.0 / 1337.2 / 1335.8 before (spread 3.2), 1334.0 /
1339.0 / 1338.3 after (-0.2 on the means); as a graph 1342.7 / 1340.5 / 1340.2 (2.5) -> 1342.7 / 1344.0 / 1343.0 (+2.1); 48 maps eager
4672.0 / 4664.1 / 4672.5 (8.4) -> 4661.6 / 4686.4 / 4677.2 (+5.5), as a graph 4601.3 / 4598.5 / 4606.1 (7.7) -> 4596.4 / 4605.6 / 4604.1
(+0.05).  Per launch at 6 maps: 3x3 bias relu 122.80 / 122.80 / 122.86 -> 122.52 / 122.78 / 123.30 (+0.05), conv1 over 1024 channels
58.0 -> 58.1 (+0.1, spread 0.1), aspp d18 45.5 -> 45.6 (+0.1), gates 37.6 -> 37.2, pool bias 32.0 -> 32.3 (+0.3, spread 0.2); at 48
maps the 1x1 launches +0.3 to +0.5 (spreads 0.2 to 0.5), the 3x3 launches +0.1 to +0.5 (spreads 0.1 to 1.6).  The compare and select
cost at most half a microsecond a launch, at or inside the parent's own spread, and no step time moved outside it.
tools/radar_pillars_bench.py (f8 shape, 200 repetitions): encode + scatter into the image 35.3 / 41.4 / 47.4 before (spread 12.1), 38.9 /
38.6 / 40.7 after; into the canvas 40.5 / 43.3 / 45.8 (5.3) -> 42.9 / 43.6 / 44.5 (+0.5 on the means); the branch 396.2 / 476.6 / 402.8 ->
402.3 / 394.1 / 405.8: nothing outside the parent's run-to-run spread.  bench.py launches none of the changed kernels: 299.3 / 299.0 /
297.1 / 300.7 / 298.9 samples/s with the parent's library, 296.1 / 298.6 / 299.6 / 299.2 / 298.7 with the fixed one, taking turns.
Two sessions on the fixed library gave the same (E_ref, kernel) figures in every digit.
"""
import ctypes
import json
import os

import pytest
import torch

import depth_net_fwd_ref as V
from racformer_amd import _lib
from racformer_amd import depth_net as DN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _p(t):
    return _lib.ptr(t) if t is not None else None


class Kernels:
    """the runner of tests/depth_net_fwd_ref.py on the device"""

    def dev(self, t):
        return t.to(DEV)

    def host(self, t):
        torch.cuda.synchronize()
        return t.cpu()

    def pack_rows(self, src, dst, c_off=0, c_pad=0, BN=None):
        assert src.is_cuda and src.is_contiguous() and dst.is_cuda and dst.is_contiguous()
        if BN is None:
            DN.pack_rows(src, dst, c_off=c_off, c_pad=c_pad)
            return 0
        n, C, hw = src.shape[:3]
        return _lib.lib().rac_conv_small_pack_fwd(_p(src), _p(dst), BN, C, hw, dst.shape[2], c_off, c_pad, _lib.stream_ptr())

    def conv_small(self, x, w, cout, H, W, BN=None, **kw):
        for t in (x, w, kw["out"]) + tuple(kw.get(k) for k in ("bias", "img_bias", "gate", "residual", "bins", "bins_table", "cls", "cls_table")):
            assert t is None or (t.is_cuda and t.is_contiguous())
        if BN is None:
            got = DN.conv_small(x, w, cout, H, W, **kw)
            assert got.data_ptr() == kw["out"].data_ptr()
            return 0
        d, out, cf = _lib.ConvSmall(), kw["out"], kw["channel_first"]
        d.in_, d.w, d.out = _p(x), _p(w), _p(out)
        for k in ("bias", "img_bias", "gate", "residual", "bins", "bins_table", "cls", "cls_table"):
            setattr(d, k, _p(kw.get(k)))
        d.BN, d.H, d.W, d.Cin, d.Cout, d.ksize, d.dilation, d.ld_in, d.ld_w = BN, H, W, kw["cin"], cout, kw["ksize"], kw["dilation"], x.shape[2], w.shape[2]
        d.gate_channels = kw["gate"].shape[-1] if kw.get("gate") is not None else 0
        d.ld_res = kw["residual"].shape[-1] if kw.get("residual") is not None else 0
        d.n_bins = kw["bins_table"].shape[0] if kw.get("bins_table") is not None else 0
        d.n_cls = kw["cls_table"].shape[0] - 1 if kw.get("cls_table") is not None else 0
        d.relu, d.out_layout = int(kw["relu"]), (_lib.CS_CHANNEL_FIRST if cf else _lib.CS_CHANNEL_LAST)
        d.ld_out, d.c_off = (out.shape[1] if cf else out.shape[2]), kw["c_off"]
        return _lib.lib().rac_conv_small_fwd(ctypes.byref(d), _lib.stream_ptr())

    def gates(self, mlp, params, out, BN, C, branches):
        assert all(t.is_cuda and t.is_contiguous() for t in (mlp, params, out)) and params.shape == (branches, V.gates_block(C))
        _lib.check(_lib.lib().rac_depthnet_gates_fwd(_p(mlp), _p(params), _p(out), BN, C, branches, _lib.stream_ptr()), "rac_depthnet_gates_fwd")

    def pool_bias(self, x, wp, bp, wb, out, BN, hw, ld, C, Cout):
        assert all(t.is_cuda and t.is_contiguous() for t in (x, wp, bp, wb, out)) and x.shape == (BN, hw, ld)
        rc = _lib.lib().rac_depthnet_pool_bias_fwd(_p(x), _p(wp), _p(bp), _p(wb), _p(out), BN, hw, ld, C, Cout, _lib.stream_ptr())
        _lib.check(rc, "rac_depthnet_pool_bias_fwd")


RUN = Kernels()


@pytest.fixture(scope="module")
def log():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    lg = V.Log()
    yield lg
    torch.set_num_threads(n)
    worst = lg.worst()
    print("\nDepthNet forwards against float64, worst per kernel and layout in units of 2^-24 x A (E_ref | kernel | err / allowed):")
    for k in sorted(worst):
        print(f"  {k:>28s}: {worst[k]['E_ref']:8.3f} | {worst[k]['kernel']:8.3f} | {worst[k]['ratio']:.4f}")
    path = os.environ.get("RAC_DEPTH_NET_FWD_ERRORS")
    if lg.errors and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(unit="2**-24", ratio_allowed=V.RATIO, floor=1.0, worst=worst, reached=sorted(lg.reached), errors=lg.errors), f, indent=1,
                      sort_keys=True)


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
    """one NaN in an input pixel, a gate, a residual element, a per-image bias or a table row: NaN exactly in the elements that read
    it (float64's set, asserted first to be the live taps' dilated footprint), with and without the ReLU behind it"""
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
    """(after the cases above) by the launchers' and kernels' rules as tests/depth_net_fwd_ref.py restates them"""
    assert V.REACH <= log.reached, sorted(V.REACH - log.reached)
