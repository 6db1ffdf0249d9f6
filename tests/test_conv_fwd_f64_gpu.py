"""The split-precision 3x3 convolution forward kernels on the MI355X against float64, element by element: rac_absmax_fwd, the three
pack kernels, conv3x3_f16x3_kernel in its five output modes and behind rac_conv3x3_temporal_fwd, conv3x3s2_c64_f16x3_kernel, the
eleven instantiations of conv_direct_kernel and rac_upsample2x_image_fwd (csrc/conv3x3.hip, conv3x3_bwd.hip, conv_direct.hip).
tests/conv_fwd_ref.py holds the cases, the references, the magnitudes, the restatements, the negative controls and the launchers'
rules restated; tests/test_conv_fwd_f64_cpu.py runs the same checks on the CPU with the restatements in the kernels' place and
shows that each of the thirteen negative controls fails its check.

Through the wrappers of racformer_amd.fused where they expose what a check needs (ConvImage.begin / pack / pack_cl / pack_live /
conv_s2 on the case's own buffers, conv_direct, upsample2x_image, quantize_values_i16); the five stride-1 entry points of
conv3x3_f16x3_kernel through the C ABI, because their wrappers (ConvImage.conv, fpn_writer, radar_pillars) allocate the destination
themselves and every destination here is a frame range of a larger NaN-filled buffer.

Stage A: rac_absmax_fwd equals max(floor, max |v|) in its bits (several sources, an empty one, n % 4 in 1..3, floors above and below
the data, the 8-deep loop, its remainder loop and the tail in one launch of 18.9 M values with the maximum in each in turn -- the
grid rule restated in absmax_paths and asserted as reached; a NaN among the values is ignored, which is what fmaxf does: asserted).
Every half-word of an image written by rac_conv_pack_fwd / rac_conv_pack_bias_fwd / rac_conv_pack_cl_fwd equals the torch
restatement at W in {1, 3, 4, 17, 128, 130, 257} (scalar and vector loads, one / two / three 128-column pieces), the border exactly
zero, the chunks outside the written range still the sentinel, live in {0, 1, 4} of 4 frames in two groups with the dead frames the
bias alone, one value 2^-20 of amax (lo a subnormal) and an all-zero source (scale 1).  Every stage B case repeats the comparison on
its own image.  Images written by an epilogue (RAC_CD_IMAGE, RAC_CD_IMAGE_RELU, the GRU's out_img, rac_upsample2x_image_fwd): value
within 2^-22 |y| + 2^-25 / scale of h_out, or of the float64 reference on top of the stage B allowance.

Stage B, per element: |got - ref| <= (4 + max(4 x E_ref, 1)) x 2^-24 x A; ref F.conv2d in float64 of the values the images hold,
A the same sum over absolute values, E_ref torch's float32 conv2d on the CPU on the same operands; A == 0 means exactly 0; NaN
exactly where float64 has NaN; the rest of every destination buffer still NaN (f16 image destinations: every half-word outside the
written frames' interior of the owned chunks unchanged).  Reached, asserted by test_everything_was_reached from the launchers' rules
restated in conv_fwd_ref.py (conv_tiles, pack_path, cd_instance): all five output modes, one and two tiles, whole and ragged last
tiles (1x1, 3x5, 16x16, 16x17, 9x29, 2x130, 16x32), 1 / 3 / 10 chunks, temporal launches with live in {0, 1, 2, 4} in both output
forms, conv3x3s2 with one and two tiles and 1 / 8 chunks, all eleven instantiations of conv_direct_kernel with whole and ragged
pixel tiles, one and two of them.  +-inf inputs are out of scope: rac_act_scale gives up on a non-finite bound by design.

Measured on the MI355X (143 tests in 4.6 s; profiles/conv_fwd_f64.json, written with RAC_CONV_FWD_ERRORS=<file>), worst over the
session in units of 2^-24 x A (E_ref | kernel) and the largest err over what the criterion allows:
  conv3x3 nhwc        3.49 | 3.54   0.50   (Cin = 320, N = 3, 16x32; the head x 1e-4, the frame x 2^-12 and the poisoned launches no worse)
  conv3x3 nchw        2.93 | 3.31   0.44   bit-equal to the channel-last result transposed in all five cases
  conv3x3 nchw_relu   2.41 | 3.13   0.39   amax given and NULL
  conv3x3 grouped     2.80 | 3.67   0.37   cams 1, 2, 3
  conv3x3 q16         mantissas and scales bit-equal to quantize_values_i16 of the channel-last output (ragged maps without a map
                      included); dequantised within the allowance + 2^-15 of the block maximum (0.92 of it: the rounding of the int16)
  conv3x3 temporal    1.58 | 4.93   0.49   live frames bit-equal to rac_conv3x3_fwd / rac_conv3x3_q16_fwd; dead frames against float64
                                           on the explicit image; q16 dequantised 0.96 of allowance + int16 rounding
  conv3x3s2           2.69 | 2.54   0.41
  direct f32 k1 / k2 / k4          2.32 | 1.83, 1.54 | 2.38, 0.90 | 2.17     0.15, 0.23, 0.29
  direct f32_cf_relu k2            1.52 | 2.67   0.31
  direct image s2 k2 / k3 / k8     1.35 | 2.05, 0.95 | 2.62, 0.61 | 2.10     0.21, 0.32, 0.30
  direct image s1 k2, image_relu   1.48 | 2.76, 1.49 | 2.82                  0.27, 0.26
  direct gru k0 / k2               0.52 | 0.52, 0.81 | 1.05                  0.29, 0.15    |h| <= 1; the image within R of h_out
  upsample2x_image                 1.44 | 3.01   0.34
No comparison is near its limit and none needed a second reference: the matrix core's 32-term sums err like a float32 chain
(kernel figures up to 4.9 against E_ref up to 3.5 over the 117 recorded pairs), and the dropped lo x lo product, which the
criterion grants 4 units, is not visible.
Power-of-two invariance (k = 20, -30), the all-zero image giving the bias, and the all-zero head giving exactly 0 or exactly the map:
bit for bit.

Found by this module and fixed with it: the ReLU epilogues of conv3x3.hip (CV_OUT_NCHW_RELU) and conv_direct.hip (EPI 1 and 2:
RAC_CD_IMAGE_RELU, RAC_CD_F32_CF_RELU) were __builtin_elementwise_max(v, 0), which returns 0 for a NaN.  Before, on the parent's
kernels, 4 of the 143 tests failed: "poison nchw_relu" and "poison nchw_relu null" each with "NaN in 0 elements where float64 has
none, none in 2304 where it has" (3x3 pixels x 256 channels came out as clean zeros), "poison image_relu" and "poison f32_cf_relu"
each with none in 576 (3x3 x 64).  After (rac_relu per component): all 143 pass; every finite result keeps its bits (-0 included:
rac_relu is fmaxf for every value but a NaN) -- golden, parity, radar-pillar and necks tests untouched and green.
Cost, tools/radar_pillars_bench.py (f8 shape, 200 repetitions, medians), the parent's and the fixed library taking turns on one
machine, three runs each, in us: radar branch total 393.6 / 399.3 / 396.4 before (spread 5.7), 396.2 / 401.9 / 400.1 after: +3.0 on
the means, inside the spread of the parent's own runs, but present in every pair (+2.6, +2.6, +3.7).  Per launch: the 64 -> 64
RAC_CD_IMAGE_RELU layer 52.9 / 52.8 / 52.9 -> 54.0 / 53.7 / 53.9 (+1.0, outside its spread of 0.1), the 64 -> 256 CV_OUT_NCHW_RELU
layer 115.6 / 116.4 / 115.9 -> 117.2 / 116.3 / 117.2 (+0.9, spread 0.8; alone 99.4 / 98.9 / 99.5 -> 100.4 / 100.2 / 100.1),
RAC_CD_F32_CF_RELU on the same layer (not the encoder's route) 158.4 / 156.4 / 158.2 -> 162.6 / 162.1 / 162.3.  The compare and
select cost about 1 us a launch, 0.75 % of the branch; recorded, and the fix is kept.  The instantiations without a ReLU compile to
the parent's instructions (device assembly of both sources compared kernel by kernel: only the three ReLU instantiations
differ), and bench.py, which launches none of the three, measures the same with either library (305.7 / 308.2 against 307.2 /
307.6 samples/s, taking turns on one machine).
Closed since (tests/test_depth_net_fwd_f64_gpu.py, tests/test_radar_pillars_gpu.py::test_2b_*): what this paragraph listed as open --
the fmaxf(v, 0) ReLUs of depth_net.hip (the convolution's epilogue, both ReLUs of the gates, the image-pool branch) and the pillar
maximum of radar_pillars.hip, which dropped a NaN point feature -- now keep a NaN (rac_relu; `y > best || y != y`).  The backbone's
ReLU (resnet.hip, v < 0 ? 0 : v) kept one already.
"""
import json
import os

import pytest
import torch

import conv_fwd_ref as V
from racformer_amd import _lib, fused

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CD_MODES = {"image": _lib.CD_IMAGE, "f32": _lib.CD_F32, "gru": _lib.CD_GRU, "image_relu": _lib.CD_IMAGE_RELU, "f32_cf_relu": _lib.CD_F32_CF_RELU}


def _p(t):
    return _lib.ptr(t) if t is not None else None


class Kernels:
    """the runner of tests/conv_fwd_ref.py on the device"""

    def dev(self, t):
        return t.to(DEV)

    def host(self, t):
        torch.cuda.synchronize()
        return t.cpu()

    def _image(self, xs, amax):
        N, Hp, Wp, chunks = xs.shape[:4]
        img = fused.ConvImage(N, Hp - 2, Wp - 2, chunks * 32, torch.device(DEV))
        img.xs, img.amax = xs, amax                      # (the case's own buffer in place of the shared scratch)
        return img

    def absmax(self, srcs, floor):
        return fused.ConvImage(1, 1, 1, 32, torch.device(DEV)).begin(list(srcs), floor).amax

    def pack(self, kind, src, amax, xs, c_offset, bias=None, T=1, live=1):
        img = self._image(xs, amax)
        if kind == "nchw":
            img.pack(src, c_offset)
        elif kind == "cl":
            img.pack_cl(src, c_offset)
        else:
            assert src.shape[0] == xs.shape[0] // T * live
            img.pack_live(src, bias, c_offset, T)

    def quantize(self, value):
        return fused.quantize_values_i16(value)

    def conv(self, kind, xs, ws, w_alpha, amax, dst, N, H, W, cin, bias=None, pmap=None, cams=1, scale=(1.0, 0.0), temporal=None):
        L, st = _lib.lib(), _lib.stream_ptr()
        q, qs = dst if kind == "q16" else (None, None)
        out = None if kind == "q16" else dst
        for t in (xs, ws, bias, pmap, out, q, qs):
            assert t is None or (t.is_cuda and t.is_contiguous())
        if temporal is not None:
            pd, cin_dead, T, live = temporal
            rc = L.rac_conv3x3_temporal_fwd(_p(xs), _p(ws), _p(pmap), _p(pd), _p(amax), float(w_alpha), _p(out), _p(q), _p(qs), N, H, W, cin,
                                            cin_dead, T, live, st)
        elif kind == "nhwc":
            rc = L.rac_conv3x3_fwd(_p(xs), _p(ws), _p(bias), _p(pmap), _p(amax), float(w_alpha), _p(out), N, H, W, cin, 256, st)
        elif kind == "q16":
            rc = L.rac_conv3x3_q16_fwd(_p(xs), _p(ws), _p(bias), _p(pmap), _p(amax), float(w_alpha), _p(q), _p(qs), N, H, W, cin, 256, st)
        elif kind == "nchw":
            rc = L.rac_conv3x3_cf_fwd(_p(xs), _p(ws), _p(bias), _p(amax), float(w_alpha), _p(out), N, H, W, cin, 256, st)
        elif kind == "nchw_relu":
            rc = L.rac_conv3x3_relu_cf_fwd(_p(xs), _p(ws), _p(bias), _p(amax), float(scale[0]), float(scale[1]), float(w_alpha), _p(out), N, H, W,
                                           cin, 256, st)
        else:
            rc = L.rac_fpn_conv_fwd(_p(xs), _p(ws), _p(bias), _p(amax), float(w_alpha), _p(out), N, H, W, cin, cams, st)
        _lib.check(rc, f"conv3x3 {kind}")

    def conv_s2(self, xs, ws, w_alpha, amax, bias, dst, N, H, W, cin, cin_image):
        assert cin_image == xs.shape[3] * 32
        got = self._image(xs, amax).conv_s2(ws, w_alpha, bias, cin, out=dst)
        assert got.data_ptr() == dst.data_ptr()

    def conv_direct(self, mode, **kw):
        fused.conv_direct(CD_MODES[mode], **kw)

    def upsample_image(self, src, img, bound):
        fused.upsample2x_image(src, img, bound)


RUN = Kernels()


@pytest.fixture(scope="module")
def log():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    lg = V.Log()
    yield lg
    torch.set_num_threads(n)
    worst = lg.worst()
    print("\n3x3 convolution forwards against float64, worst per kernel and mode in units of 2^-24 x A (E_ref | kernel | err / allowed):")
    for k in sorted(worst):
        print(f"  {k:>28s}: {worst[k]['E_ref']:8.3f} | {worst[k]['kernel']:8.3f} | {worst[k]['ratio']:.4f}")
    path = os.environ.get("RAC_CONV_FWD_ERRORS")
    if lg.errors and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(unit="2**-24", ratio_allowed=V.RATIO, lo_lo=V.LOLO, floor=1.0, worst=worst, reached=sorted(lg.reached), errors=lg.errors), f,
                      indent=1, sort_keys=True)


def test_absmax():
    assert V.check_absmax(RUN) == {"deep", "single", "tail"}


@pytest.mark.parametrize("W", V.PACK_WIDTHS)
@pytest.mark.parametrize("kind", V.PACK_KINDS)
def test_pack(kind, W):
    V.check_pack(RUN, kind, W)


@pytest.mark.parametrize("magnitude", ["tiny", "zero"])
@pytest.mark.parametrize("kind,W", [("nchw", 17), ("nchw", 128), ("cl", 17), ("live1", 4), ("live4", 130)])
def test_pack_magnitudes(kind, W, magnitude):
    V.check_pack(RUN, kind, W, magnitude)


@pytest.mark.parametrize("name", V.CONV_PLAIN)
def test_conv3x3(log, name):
    V.check_conv(log, name, RUN)


@pytest.mark.parametrize("name", V.CONV_POISON)
def test_conv3x3_poisoned(log, name):
    """one NaN in the input of one frame: NaN on float64's 3x3 footprint in every output channel of that frame and nowhere else;
    the ReLU mode behind it keeps the NaN as torch.relu does"""
    V.check_conv_poison(log, name, RUN)


@pytest.mark.parametrize("name", list(V.TEMPORAL_CASES))
def test_temporal(log, name):
    V.check_temporal(log, name, RUN)


@pytest.mark.parametrize("name", list(V.S2_CASES))
def test_conv3x3s2(log, name):
    V.check_s2(log, name, RUN)


@pytest.mark.parametrize("name", V.DIRECT_PLAIN)
def test_conv_direct(log, name):
    V.check_direct(log, name, RUN)


@pytest.mark.parametrize("name", V.DIRECT_POISON)
def test_conv_direct_poisoned(log, name):
    V.check_direct(log, name, RUN)


@pytest.mark.parametrize("name", list(V.UPSAMPLE_CASES))
def test_upsample_image(log, name):
    V.check_upsample(log, name, RUN)


def test_everything_was_reached(log):
    """(after the cases above) every output mode, tile shape and chunk count, and all eleven instantiations of conv_direct_kernel,
    by the launchers' rules as tests/conv_fwd_ref.py restates them"""
    assert V.REACH <= log.reached, sorted(V.REACH - log.reached)
