"""The float64 criterion for the split-precision 3x3 convolution forward kernels (csrc/conv3x3.hip: absmax_kernel, conv_pack_kernel,
conv3x3_f16x3_kernel in its five output modes, conv3x3s2_c64_f16x3_kernel; csrc/conv3x3_bwd.hip: conv_pack_cl_kernel;
csrc/conv_direct.hip: the eleven instantiations of conv_direct_kernel, upsample2x_image_kernel): cases, references, magnitudes,
restatements, negative controls and the launchers' rules, shared by tests/test_conv_fwd_f64_cpu.py and
tests/test_conv_fwd_f64_gpu.py (test helper, no GPU).

The thing under test is a ``runner``: an object with
  dev(t) / host(t)                                   a CPU tensor onto the runner's device and back
  absmax(srcs, floor)                                -> amax [1]                                        (rac_absmax_fwd)
  pack(kind, src, amax, xs, c_offset, bias, T, live) kind "nchw" / "live" / "cl": writes a channel range of the image xs
  conv(kind, xs, ws, w_alpha, amax, dst, N, H, W, cin, bias, pmap, cams, scale, temporal)
                                                     kind "nhwc" / "nchw" / "nchw_relu" / "grouped" / "q16": writes dst
  conv_s2(xs, ws, w_alpha, amax, bias, dst, N, H, W, cin, cin_image)
  conv_direct(mode, **kw)                            racformer_amd.fused.conv_direct's keywords, mode "image" / "image_relu" /
                                                     "f32" / "f32_cf_relu" / "gru"
  upsample_image(src, img, bound)                    rac_upsample2x_image_fwd
  quantize(value)                                    -> (q, scale)                                      (rac_quant_i16_fwd)
``Restated`` is the runner of the CPU module: the kernels' arithmetic in float32 torch (the three kept products hi hi + hi lo +
lo hi as three float32 convolutions of the half-words, the power-of-two unscale, the epilogue); with ``fault=`` it is each of the
negative controls (FAULTS).

Stage A, the operands, bit for bit.  Pack arithmetic is deterministic -- v * 2^e exactly, hi = f16(v 2^e) to nearest, the exact
difference, lo = f16 of it -- so the image a pack kernel writes equals ``Restated().pack`` in every half-word: the written channel
range, the zero border, and the sentinel the other chunks were filled with.  rac_absmax_fwd equals max(floor, max |v|) in its bits,
a NaN among the values being ignored (fmaxf returns its other argument).  Every stage B case repeats that check on its own image
before the image is used, which is also what lets the float64 reference of a case be computed once and shared.
An image written by a kernel's epilogue cannot be restated in its bits (fma, expf, tanhf); its value (hi + lo) / scale lies within
    R = 2^-22 |y| + 2^-25 / scale
of the float32 value y stored beside it (the GRU's h_out), or of the float64 reference where nothing is stored beside it (then on
top of the stage B allowance): lo's rounding is 2^-11 of |lo| <= 2^-11 |y|, and below f16's normal range lo's step is 2^-24.

Stage B, every output element against float64.  The reference is F.conv2d in float64 of the values the two images hold,
X = (hi + lo) / scale and Wv = unpack_conv3x3_weight(ws, w_alpha), plus bias or per-pixel map; pack errors do not enter.
    |got - ref| <= (4 + max(4 E_ref, 1)) 2^-24 A,         A = conv(|X|, |Wv|) + |bias| + |map|
4: the dropped lo x lo product (|x_lo| <= 2^-11 |x|, |w_lo| <= 2^-11 |w|: 2^-22 of A).  E_ref: the worst err / A, in 2^-24, of
torch's float32 conv2d on the CPU on the same X and Wv (both exact in float32).  An element with A == 0 is exactly 0; NaN exactly
where float64 has NaN; no element is left out.  Every fp32 destination is a frame range (conv_s2: also a channel range) of a larger
NaN-filled buffer whose remainder must still be NaN; an f16 image destination starts from zeros with a sentinel in the chunks the
launch does not own, and everything outside the written frames' interior of the owned chunks keeps its bits.
The GRU: the float64 gate formula (models/racformer_transformer.py:714-720) on the image's own values; A carried through the
gates with the derivative bounds sigmoid' <= 1/4, tanh' <= 1 times the pre-activations' A, plus each intermediate's own size for
its rounding; E_ref from the same formula in float32.
rac_upsample2x_image_fwd: rowwise_ref.upsample64, the magnitude with the tap position's two roundings, plus R.
+-inf inputs are out of scope: rac_act_scale gives up on a non-finite bound by design (scale 1)."""
import functools
import math

import torch
import torch.nn.functional as TF

from racformer_amd.fused import pack_conv3x3_weight, unpack_conv3x3_weight
from racformer_amd.transformer import dead_frame_bias_map
from rowwise_ref import F32, F64, NAN, TINY, U, OutOfBound, bits_equal, upsample64

F16 = torch.float16
RATIO, LOLO = 4.0, 4.0
SENTINEL = 77.0                      # f16 value of the image chunks a launch does not own
Q_SENTINEL = -32768                  # an int16 the quantiser never writes (it clamps to +-32767)
CV_TM, S2_TM, COUT = 256, 128, 256
ABSMAX_BLOCK_CAP = 2048


# --------------------------------------------------------------------------------------------- host forms of device helpers
def f32(v):
    return float(torch.tensor(float(v), dtype=F32))


def act_scale(bound):
    """rac_act_scale (csrc/rac_common.h): the power of two that brings ``bound`` into [2^13, 2^14); 1 for 0 / tiny / non-finite"""
    b = f32(bound)
    if not b > f32(1.0e-30) or not b < f32(3.0e38):
        return 1.0
    return 2.0 ** (14 - math.frexp(b)[1])


def bound32(amax, mul, add):
    """rac_cd_scale's expression in float32: (amax ? mul * amax : 0) + add"""
    return f32((f32(f32(mul) * f32(amax)) if amax is not None else 0.0) + f32(add))


def cd_frame(fr, n, fault=None):
    live, stride, first = fr
    if fault == "frame_map_div_mod_swapped":
        return (n % live) * stride + n // live + first
    return (n // live) * stride + n % live + first


def split_f16(v):
    """f32 -> (hi, lo), both f16, round to nearest"""
    v = v.float()
    hi = v.half()
    return hi, (v - hi.float()).half()


def image_put(xs, hi, lo, chunk0):
    """hi / lo [N,C,H,W] f16 -> the interior pixels of chunks chunk0.. of xs [N,H+2,W+2,chunks,2,32]"""
    N, C, H, W = hi.shape
    v = torch.stack([hi.reshape(N, C // 32, 32, H, W), lo.reshape(N, C // 32, 32, H, W)], 2)     # [N, ch, 2, 32, H, W]
    xs[:, 1:-1, 1:-1, chunk0:chunk0 + C // 32] = v.permute(0, 4, 5, 1, 2, 3)


def image_halves(xs, dtype=F32):
    """xs [N,H+2,W+2,chunks,2,32] -> (hi, lo) [N,C,H+2,W+2]"""
    N, Hp, Wp, ch = xs.shape[:4]
    return tuple(xs[..., k, :].to(dtype).reshape(N, Hp, Wp, ch * 32).permute(0, 3, 1, 2).contiguous() for k in (0, 1))


def image_values(xs, scale, dtype=F64):
    """the values an image holds, border included: [N,C,H+2,W+2]"""
    hi, lo = image_halves(xs, dtype)
    return (hi + lo) / scale


def weight_halves(ws):
    """ws [9,chunks,cout,2,32] f16 -> (hi, lo) [cout, Cin, 3, 3] f32, still times 2^s"""
    taps, chunks, co = ws.shape[:3]
    return tuple(ws[:, :, :, k].float().permute(2, 1, 3, 0).reshape(co, chunks * 32, 3, 3).contiguous() for k in (0, 1))


def image_equal(a, b):
    """bit for bit, except that any NaN matches any NaN"""
    a, b = a.contiguous(), b.contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {F16: torch.int16, F32: torch.int32}[a.dtype]
    return bool(((a.view(it) == b.view(it)) | (torch.isnan(a) & torch.isnan(b))).all())


def quantize_host(value):
    """rac_quant_i16_fwd / the CV_OUT_Q16 epilogue: [..., 64] f32 -> (int16 mantissas, [...] f32 power-of-two scales); a block whose
    maximum is inf or NaN gets a NaN scale"""
    bits = value.contiguous().view(torch.int32) & 0x7fffffff
    eb = (bits.max(-1).values >> 23) & 255
    bad = eb == 255
    eb = eb.clamp(min=15)
    up = torch.where(bad, torch.zeros((), dtype=F64), torch.pow(2.0, (141 - eb).double())).float()
    dn = torch.where(bad, torch.full((), NAN, dtype=F64), torch.pow(2.0, (eb - 141).double())).float()
    q = torch.round(value * up.unsqueeze(-1))
    q = torch.where(torch.isnan(q), torch.full_like(q, -32767.0), q).clamp(-32767.0, 32767.0)
    return q.to(torch.int16), dn


# ------------------------------------------------------------------------------------------- the launchers' rules, restated
def absmax_paths(n):
    """which of absmax_kernel's three loops a source of n floats reaches: blocks = clamp(ceil(n/4 / 256), 1, 2048), a thread starts at
    float4 i < stride = 256 blocks, takes eight per trip while i + 7 stride < n/4, then one per trip, and block 0 the n % 4 tail"""
    n4 = n // 4
    stride = 256 * max(1, min(ABSMAX_BLOCK_CAP, (n4 + 255) // 256))
    deep = n4 > 7 * stride
    trips = (n4 - 7 * stride + 8 * stride - 1) // (8 * stride) if deep else 0          # of thread 0
    return dict(deep=deep, single=n4 > 8 * stride * trips, tail=n % 4 != 0)


def pack_path(W):
    """conv_pack_kernel: (vector or scalar loads, number of 128-column pieces of a row)"""
    return ("vector" if W % 4 == 0 else "scalar"), (W + 127) // 128


def conv_tiles(H, W):
    """conv3x3_f16x3_kernel: (tiles of 256 pixels per image, valid pixels of the last one)"""
    t = (H * W + CV_TM - 1) // CV_TM
    return t, H * W - (t - 1) * CV_TM


CD_INSTANCES = ("gru k0", "gru k2", "image s2 k2", "image s2 k3", "image s2 k8", "image s1 k2", "image_relu s1 k2", "f32 k1", "f32 k2",
                "f32 k4", "f32_cf_relu k2")


def cd_instance(mode, stride, chunks):
    """rac_conv_direct_fwd's dispatch -> (the instantiation's name, pixels per workgroup = 64 PT); None where it refuses"""
    if mode == "gru":
        return (f"gru k{chunks}", 64) if stride == 1 and chunks in (0, 2) else None
    if mode == "image" and stride == 2:
        return (f"image s2 k{chunks}", 64) if chunks in (2, 3, 8) else None
    if mode in ("image", "image_relu"):
        return (f"{mode} s1 k2", 256) if stride == 1 and chunks == 2 else None
    if mode == "f32_cf_relu":
        return ("f32_cf_relu k2", 128) if stride == 1 and chunks == 2 else None
    if mode == "f32":
        return (f"f32 k{chunks}", 128) if stride == 1 and chunks in (1, 2, 4) else None
    return None


# ------------------------------------------------------------------------------------------------------------- the metric
def bound_of(e_ref):
    return LOLO + max(RATIO * e_ref, 1.0)


class Log:
    """every (E_ref, kernel) pair of a session, keyed "<kernel and mode> | <case> | <output>", in units of 2^-24 of A; ``ratio`` the
    worst err over what the criterion allows at that element; ``compare`` prints, then asserts.  ``reached``: the instantiations
    and paths the session's launches took, by the launchers' rules restated above."""

    def __init__(self):
        self.errors, self.reached = {}, set()

    def compare(self, key, got, ref, A, r32, R=None, lolo=True):
        got, ref, A, r32 = (t.detach().double() for t in (got, ref, A, r32))
        R = torch.zeros_like(A) if R is None else R.double()
        assert got.shape == ref.shape == A.shape == r32.shape == R.shape, (key, got.shape, ref.shape, A.shape, r32.shape)
        nan = torch.isnan(ref)
        ok = ~nan
        assert bool(torch.isfinite(ref[ok]).all()) and bool(torch.isfinite(A[ok]).all()), f"{key}: the reference is not finite"
        if not torch.equal(torch.isnan(got), nan):
            raise OutOfBound(f"{key}: NaN in {int((torch.isnan(got) & ok).sum())} elements where float64 has none, "
                             f"none in {int((~torch.isnan(got) & nan).sum())} where it has")
        if not bool((got[ok & (A == 0) & (R == 0)] == 0).all()):
            raise OutOfBound(f"{key}: an element of magnitude 0 is not exactly 0")
        live = ok & (A > 0)
        e_ref = float(((r32 - ref).abs()[live] / A[live]).max() / U) if bool(live.any()) else 0.0
        bound = bound_of(e_ref) if lolo else max(RATIO * e_ref, 1.0)
        err, allowed = (got - ref).abs(), bound * U * A + R
        kernel = ratio = 0.0
        if bool(live.any()):
            kernel = float(torch.where(live, err / A.clamp(min=TINY), torch.zeros_like(err)).max() / U)
            ratio = float(torch.where(ok, err / allowed.clamp(min=TINY), torch.zeros_like(err)).max())
        self.errors[key] = dict(E_ref=e_ref, kernel=kernel, allowed=bound, ratio=ratio)
        print(f"{key}: E_ref {e_ref:.3g}, kernel {kernel:.3g} (allowed {bound:.3g}{' + R' if bool((R > 0).any()) else ''}) x 2^-24; "
              f"worst err / allowed {ratio:.3g}")
        bad = ok & ~(err <= allowed + TINY)
        if bool(bad.any()):
            raise OutOfBound(f"{key}: {int(bad.sum())} elements above ({LOLO:g} + max({RATIO:g} x E_ref {e_ref:.3g}, 1)) x 2^-24 x A; "
                             f"worst err / allowed {ratio:.3g}")
        return bound

    def worst(self):
        """kernel and mode -> the session's worst E_ref, kernel figure and err / allowed"""
        out = {}
        for key, e in self.errors.items():
            w = out.setdefault(key.split(" | ")[0], dict(E_ref=0.0, kernel=0.0, ratio=0.0))
            for k in w:
                w[k] = max(w[k], e[k])
        return out


def require(cond, msg):
    """a bit-for-bit requirement (OutOfBound: what a negative control may also trip)"""
    if not cond:
        raise OutOfBound(msg)


# ---------------------------------------------------------------------------------------------------------- guarded buffers
def guarded(run, frames, rest, lead=2, trail=1, dtype=F32, fill=NAN):
    """-> (a [lead + frames + trail, *rest] buffer of the sentinel on the device, the [frames, *rest] region a kernel may write)"""
    full = run.dev(torch.full((lead + frames + trail,) + tuple(rest), fill, dtype=dtype))
    return full, full[lead:lead + frames]


def taken(run, full, frames, lead=2, fill=NAN):
    """the region's content on the host, after asserting that the remainder still is the sentinel"""
    full = run.host(full)
    rest = torch.cat([full[:lead].flatten(), full[lead + frames:].flatten()])
    assert bool(torch.isnan(rest).all() if fill != fill else (rest == fill).all()), "a kernel wrote outside its destination"
    return full[lead:lead + frames]


# =============================================================================================== stage A: absmax and pack
ABSMAX_BIG = 4 * (9 * 256 * ABSMAX_BLOCK_CAP + 100) + 3          # all three loops in one launch


def check_absmax(run):
    """-> the set of loops reached"""
    g = torch.Generator().manual_seed(11)
    reached = set()
    # several sources, a zero-length one, counts with n % 4 in 1..3, the maximum in a tail, a NaN among the values
    buf = torch.randn(4096, generator=g)
    for counts in ((1,), (2, 0, 3), (5, 1026, 0, 7), (1024, 259)):
        srcs, off = [], 0
        for n in counts:
            srcs.append(buf[off:off + n].clone())
            off += (n + 3) // 4 * 4 + 4
        for where in ("plain", "tail", "nan"):
            ss = [s.clone() for s in srcs]
            last = max(i for i, n in enumerate(counts) if n)
            if where == "tail" and counts[last] % 4:
                ss[last][-1] = -9.5
            if where == "nan":
                ss[last][counts[last] // 2] = NAN
            for floor in (0.0, 0.125, 50.0):
                got = run.host(run.absmax([run.dev(s) for s in ss], floor))
                want = Restated().absmax(ss, floor)
                require(bits_equal(got.view(1), want.view(1)), f"absmax {counts} {where} floor {floor}: {float(got)} != {float(want)}")
                for n in counts:
                    reached |= {k for k, v in absmax_paths(n).items() if v and n}
    # the NaN is ignored: what fmaxf does, and what the restatement asserts above; stated on its own
    s = torch.tensor([1.0, NAN, -3.0, 2.0, NAN])
    require(float(run.host(run.absmax([run.dev(s)], 0.0))) == 3.0, "absmax: a NaN is not ignored")
    # the 8-deep loop, its remainder loop and the tail in one launch, the maximum in each of them in turn
    n = ABSMAX_BIG
    p = absmax_paths(n)
    assert p == dict(deep=True, single=True, tail=True), p
    big = torch.randn(n, generator=g)
    stride4 = 4 * 256 * ABSMAX_BLOCK_CAP
    for pos in (3 * stride4 + 1234, 8 * stride4 + 4 * 77 + 2, n - 1, None):
        b = big.clone()
        if pos is not None:
            b[pos] = -123.5
        got = run.host(run.absmax([run.dev(b)], 1.0))
        require(float(got) == float(b.abs().max()), f"absmax of {n} values, maximum at {pos}: {float(got)}")
    return reached | {k for k, v in p.items() if v}


PACK_WIDTHS = (1, 3, 4, 17, 128, 130, 257)
PACK_KINDS = ("nchw", "cl", "live0", "live1", "live4")


def pack_case(kind, W, magnitude="plain"):
    """a pack launch: C = 64 channels into chunks 1..2 of a 4-chunk image, H = 3 rows (2 for the wide ones)"""
    T = 4 if kind.startswith("live") else 1
    live = int(kind[4:]) if T == 4 else 1
    N, C, H = (2 * T if T == 4 else 2), 64, (3 if W < 128 else 2)
    g = torch.Generator().manual_seed(100 + W + 7 * PACK_KINDS.index(kind))
    src = torch.randn((N // T) * live, C, H, W, generator=g) * 3.0
    bias = torch.randn(C, generator=g) if T == 4 else None
    if magnitude == "zero":
        src.zero_()
        bias = None if bias is None else torch.zeros_like(bias)
    scan = [src] + ([bias] if bias is not None else [])
    floor = float(src.abs().max() + bias.abs().max()) if bias is not None and src.numel() else 0.0
    if magnitude == "tiny" and src.numel():                      # one value 2^-20 of amax: its lo half is an f16 subnormal
        amax = max(float(src.abs().max()), floor)
        src.view(-1)[src.numel() // 3] = amax * 2.0 ** -20 * 1.2345
        if bias is not None:                                     # (no bias on that channel: the image holds the value itself)
            bias[(src.numel() // 3 // (H * W)) % C] = 0
    if kind == "cl":
        src = src.permute(0, 2, 3, 1).contiguous()
    return dict(kind=kind, N=N, C=C, H=H, W=W, T=T, live=live, src=src, bias=bias, scan=scan, floor=floor)


def check_pack(run, kind, W, magnitude="plain"):
    c = pack_case(kind, W, magnitude)
    N, H = c["N"], c["H"]
    before = torch.zeros(N, H + 2, W + 2, 4, 2, 32, dtype=F16)
    before[:, :, :, [0, 3]] = SENTINEL
    amax = run.absmax([run.dev(s) for s in c["scan"]], c["floor"])
    amax_h = run.host(amax)
    require(bits_equal(amax_h.view(1), Restated().absmax(c["scan"], c["floor"]).view(1)), f"pack {kind} W{W}: amax")
    if magnitude == "zero":
        assert float(amax_h) == 0.0 and act_scale(float(amax_h)) == 1.0
    xs = run.dev(before.clone())
    pk = "live" if c["T"] == 4 else kind
    run.pack(pk, run.dev(c["src"]), amax, xs, 32, run.dev(c["bias"]) if c["bias"] is not None else None, c["T"], c["live"])
    want = before.clone()
    Restated().pack(pk, c["src"], amax_h, want, 32, c["bias"], c["T"], c["live"])
    got = run.host(xs)
    # (one comparison of the whole buffer: the written range, its zero border, and the sentinel of chunks 0 and 3)
    bad = got.view(torch.int16) != want.view(torch.int16)
    require(not bool(bad.any()), f"pack {kind} W{W} {magnitude}: {int(bad.sum())} half-words differ "
                                 f"({int(bad[:, 1:-1, 1:-1, 1:3].sum())} inside the written range)")
    if magnitude == "tiny":
        lo = want[:, 1:-1, 1:-1, 1:3, 1].float().abs()
        assert bool(((lo > 0) & (lo < 2.0 ** -14)).any()), "no subnormal lo half in the image"
    if c["T"] == 4 and c["live"] < 4 and magnitude == "plain":         # dead frames: the bias alone
        sc = act_scale(float(amax_h))
        hi, lo = split_f16(c["bias"] * sc)
        dead = got.view(2, 4, H + 2, W + 2, 4, 2, 32)[:, c["live"]:, 1:-1, 1:-1, 1:3]
        assert bits_equal(dead[..., 0, :].reshape(-1, 64), hi.expand(dead[..., 0, :].reshape(-1, 64).shape).contiguous())
        assert bits_equal(dead[..., 1, :].reshape(-1, 64), lo.expand(dead[..., 1, :].reshape(-1, 64).shape).contiguous())
    return pack_path(W)


# =============================================================================================== stage B: conv3x3_f16x3_kernel
MAPS = ((1, 1), (3, 5), (16, 16), (16, 17), (9, 29), (2, 130), (16, 32))
CONV_KINDS = ("nhwc", "nchw", "nchw_relu", "grouped", "q16")


def _conv_cases():
    c = {}
    for i, (H, W) in enumerate(MAPS):
        c[f"nhwc bias {H}x{W}"] = dict(kind="nhwc", H=H, W=W, N=(1, 3)[i % 2], cin=(32, 96, 320)[i % 3])
    c["nhwc bias 16x32 N3 C320"] = dict(kind="nhwc", H=16, W=32, N=3, cin=320)
    c["nhwc no bias 9x29"] = dict(kind="nhwc", H=9, W=29, N=3, cin=96, bias=False)
    c["nhwc no bias 1x1"] = dict(kind="nhwc", H=1, W=1, N=3, cin=32, bias=False)
    c["nhwc map 16x16"] = dict(kind="nhwc", H=16, W=16, N=3, cin=32, pmap=True)
    c["nhwc map 16x32"] = dict(kind="nhwc", H=16, W=32, N=1, cin=320, pmap=True)
    for H, W, N, cin in ((16, 17, 3, 96), (2, 130, 1, 32), (1, 1, 3, 32), (16, 32, 1, 320), (3, 5, 1, 96)):
        c[f"nchw {H}x{W}"] = dict(kind="nchw", H=H, W=W, N=N, cin=cin, also_nhwc=True)
    c["nchw_relu amax 9x29"] = dict(kind="nchw_relu", H=9, W=29, N=3, cin=96, scale=(2.0, 0.5))
    c["nchw_relu amax 16x32"] = dict(kind="nchw_relu", H=16, W=32, N=1, cin=320, scale=(1.0, 0.0))
    c["nchw_relu null 16x17"] = dict(kind="nchw_relu", H=16, W=17, N=1, cin=32, scale=(None, 6.0))
    c["nchw_relu null 3x5"] = dict(kind="nchw_relu", H=3, W=5, N=3, cin=96, scale=(None, 8.0))
    for cams in (1, 2, 3):
        c[f"grouped cams{cams} 9x29"] = dict(kind="grouped", H=9, W=29, N=6, cin=(32, 96, 32)[cams - 1], cams=cams)
    c["grouped cams2 16x16"] = dict(kind="grouped", H=16, W=16, N=6, cin=32, cams=2, bias=False)
    c["q16 9x29"] = dict(kind="q16", H=9, W=29, N=3, cin=96)
    c["q16 16x17 no bias"] = dict(kind="q16", H=16, W=17, N=1, cin=32, bias=False)
    c["q16 map 16x16"] = dict(kind="q16", H=16, W=16, N=3, cin=32, pmap=True)
    c["heads 16x17"] = dict(kind="nhwc", H=16, W=17, N=1, cin=96, heads=True)
    c["heads map 16x16"] = dict(kind="nhwc", H=16, W=16, N=3, cin=32, heads=True, pmap=True)
    c["heads nchw_relu 9x29"] = dict(kind="nchw_relu", H=9, W=29, N=1, cin=32, heads=True, scale=(1.0, 0.0))
    c["small frame 16x17"] = dict(kind="nhwc", H=16, W=17, N=3, cin=96, small_frame=1, bias=False)
    c["small frame grouped 9x29"] = dict(kind="grouped", H=9, W=29, N=6, cin=32, cams=3, small_frame=4, bias=False)
    for k in (20, -30):
        c[f"pow2 k{k}"] = dict(kind="nhwc", H=9, W=29, N=1, cin=32, bias=False, pow2=k)
    c["zero image 3x5"] = dict(kind="nhwc", H=3, W=5, N=1, cin=32, zero=True)
    c["zero image nchw 16x17"] = dict(kind="nchw", H=16, W=17, N=3, cin=96, zero=True)
    for kind in CONV_KINDS:
        c[f"poison {kind}"] = dict(kind=kind, H=9, W=29, N=3 if kind != "grouped" else 6, cin=96, poison=True, cams=3 if kind == "grouped" else 1,
                                   scale=(2.0, 0.5) if kind == "nchw_relu" else None)
    c["poison nchw_relu null"] = dict(kind="nchw_relu", H=16, W=17, N=3, cin=96, poison=True, scale=(None, 6.0))
    c["poison nhwc map"] = dict(kind="nhwc", H=16, W=32, N=3, cin=96, poison=True, pmap=True)
    return c


CONV_CASES = _conv_cases()
CONV_PLAIN = [n for n, s in CONV_CASES.items() if not s.get("poison")]
CONV_POISON = [n for n, s in CONV_CASES.items() if s.get("poison")]
POISON_AT = dict(frame=1, channel=37)


@functools.lru_cache(maxsize=None)
def conv_case(name):
    s = CONV_CASES[name]
    N, H, W, cin = s["N"], s["H"], s["W"], s["cin"]
    g = torch.Generator().manual_seed(1000 + list(CONV_CASES).index(name))
    x = torch.randn(N, cin, H, W, generator=g)
    weight = torch.randn(COUT, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
    bias = torch.randn(COUT, generator=g) * 0.3 if s.get("bias", True) and not s.get("pmap") else None
    pmap = torch.randn(H * W, COUT, generator=g) if s.get("pmap") else None
    if s.get("heads"):                                   # channels 0..63 small, 64..127 exactly zero with zero bias
        weight[:64] *= 1.0e-4
        weight[64:128] = 0
        if bias is not None:
            bias[64:128] = 0
    if "small_frame" in s:
        x[s["small_frame"]] *= 2.0 ** -12
    if s.get("zero"):
        x.zero_()
    if "pow2" in s:
        x = x * 2.0 ** s["pow2"]
    poisoned = None
    if s.get("poison"):
        poisoned = (POISON_AT["frame"], POISON_AT["channel"], H // 2, W - 2)
        x[poisoned] = NAN
    ws, w_alpha = pack_conv3x3_weight(weight)
    return dict(name=name, kind=s["kind"], N=N, H=H, W=W, cin=cin, x=x, ws=ws, w_alpha=w_alpha, bias=bias, pmap=pmap, cams=s.get("cams", 1),
                scale=s.get("scale"), spec=s, poisoned=poisoned)


def _addend(c, dtype):
    if c["pmap"] is not None:
        return c["pmap"].to(dtype).t().reshape(1, COUT, c["H"], c["W"])
    if c["bias"] is not None:
        return c["bias"].to(dtype).view(1, COUT, 1, 1)
    return torch.zeros(1, COUT, 1, 1, dtype=dtype)


def image_bound(c):
    """-> (amax as rac_absmax_fwd gives it, the bound the image is packed with): amax itself, or the derived bound of the ReLU mode"""
    amax = float(Restated().absmax([c["x"]], 0.0))
    if c["scale"] is None:
        return amax, amax
    mul, add = c["scale"]
    return amax, bound32(amax if mul is not None else None, mul or 0.0, add)


@functools.lru_cache(maxsize=None)
def conv_reference(name):
    """-> the image as the pack restatement makes it, and ref (float64), A, r32 (torch's float32 conv2d), all [N,256,H,W]; read-only"""
    c = conv_case(name)
    N, H, W, cin = c["N"], c["H"], c["W"], c["cin"]
    amax, bound = image_bound(c)
    xs = torch.zeros(N, H + 2, W + 2, cin // 32, 2, 32, dtype=F16)
    Restated().pack("nchw", c["x"], torch.tensor([bound]), xs, 0)
    X, Wv = image_values(xs, act_scale(bound)), unpack_conv3x3_weight(c["ws"], c["w_alpha"])
    with torch.no_grad():
        ref = TF.conv2d(X, Wv) + _addend(c, F64)
        A = TF.conv2d(torch.nan_to_num(X.abs()), Wv.abs()) + _addend(c, F64).abs()
        r32 = TF.conv2d(X.float(), Wv.float()) + _addend(c, F32)
        if c["kind"] == "nchw_relu":
            ref, r32 = torch.relu(ref), torch.relu(r32)
    return dict(xs=xs, amax=amax, bound=bound, ref=ref, A=A.expand_as(ref).contiguous(), r32=r32)


def device_image(run, c, r):
    """the case's image made on the runner's device (absmax, pack), compared with the restatement's in every half-word
    -> (xs, the amax word the convolution reads, (scale_mul, scale_add) of the ReLU mode)"""
    N, H, W, cin = c["N"], c["H"], c["W"], c["cin"]
    x = run.dev(c["x"])
    amax = run.absmax([x], 0.0)
    require(f32(float(run.host(amax))) == f32(r["amax"]), f"{c['name']}: amax {float(run.host(amax))} != {r['amax']}")
    xs = run.dev(torch.zeros(N, H + 2, W + 2, cin // 32, 2, 32, dtype=F16))
    scale = (1.0, 0.0)
    if c["scale"] is None:
        run.pack("nchw", x, amax, xs, 0)
    else:
        run.pack("nchw", x, run.dev(torch.tensor([r["bound"]])), xs, 0)
        mul, add = c["scale"]
        amax, scale = (amax, (mul, add)) if mul is not None else (None, (0.0, add))
    require(image_equal(run.host(xs), r["xs"]), f"{c['name']}: the packed image differs from the restatement")
    return xs, amax, scale


def dst_shape(kind, N, H, W, cams=1):
    """-> (frames, rest) of a mode's fp32 destination"""
    return {"nhwc": (N, (H, W, COUT)), "nchw": (N, (COUT, H * W)), "nchw_relu": (N, (COUT, H * W)),
            "grouped": (N // cams * 4, (cams, H * W, 64))}[kind]


def canon(kind, out, N, H, W, cams=1):
    """a mode's destination layout -> [N,256,H,W]"""
    if kind == "nhwc":
        return out.permute(0, 3, 1, 2)
    if kind in ("nchw", "nchw_relu"):
        return out.reshape(N, COUT, H, W)
    return out.reshape(N // cams, 4, cams, H * W, 64).permute(0, 2, 1, 4, 3).reshape(N, COUT, H, W)      # n = bt * cams + cam, co = g * 64 + c


def launch_conv(run, c, kind, xs, amax, scale, temporal=None, ws=None):
    """one launch into a guarded destination -> [N,256,H,W] on the host (q16: (q [N,HW,4,64], scale [N,HW,4]))"""
    N, H, W, cin = c["N"], c["H"], c["W"], c["cin"]
    ws = run.dev(c["ws"] if ws is None else ws)
    bias = run.dev(c["bias"]) if c["bias"] is not None else None
    pmap = run.dev(c["pmap"]) if c["pmap"] is not None else None
    if temporal is not None:
        temporal = (run.dev(temporal[0]),) + tuple(temporal[1:])
    if kind == "q16":
        qf, q = guarded(run, N, (H * W, 4, 64), dtype=torch.int16, fill=Q_SENTINEL)
        sf, sc = guarded(run, N, (H * W, 4))
        run.conv(kind, xs, ws, c["w_alpha"], amax, (q, sc), N, H, W, cin, bias=bias, pmap=pmap, temporal=temporal)
        return taken(run, qf, N, fill=Q_SENTINEL), taken(run, sf, N)
    frames, rest = dst_shape(kind, N, H, W, c["cams"])
    full, dst = guarded(run, frames, rest)
    run.conv(kind, xs, ws, c["w_alpha"], amax, dst, N, H, W, cin, bias=bias, pmap=pmap, cams=c["cams"], scale=scale, temporal=temporal)
    return canon(kind, taken(run, full, frames), N, H, W, c["cams"])


def check_q16(run, c, key, q, sc, nhwc):
    """mantissas and scales bit-equal to rac_quant_i16_fwd of the channel-last fp32 output"""
    N, H, W = c["N"], c["H"], c["W"]
    wq, wsc = run.quantize(run.dev(nhwc.permute(0, 2, 3, 1).reshape(N, H * W, 4, 64).contiguous()))
    wq, wsc = run.host(wq), run.host(wsc)
    require(image_equal(sc, wsc), f"{key}: the int16 blocks' scales differ from quantize_values_i16 of the fp32 output")
    require(torch.equal(q, wq), f"{key}: {int((q != wq).sum())} mantissas differ from quantize_values_i16 of the fp32 output")
    require(torch.equal(q, quantize_host(nhwc.permute(0, 2, 3, 1).reshape(N, H * W, 4, 64).contiguous())[0]), f"{key}: mantissas differ from the host form")


def check_conv(log, name, run):
    """one case of conv3x3_f16x3_kernel against float64, with what its flags add"""
    c, r = conv_case(name), conv_reference(name)
    s, kind, N, H, W = c["spec"], c["kind"], c["N"], c["H"], c["W"]
    key = f"conv3x3 {kind} | {name}"
    xs, amax, scale = device_image(run, c, r)
    tiles, last = conv_tiles(H, W)
    log.reached |= {f"conv3x3 {kind}", f"conv3x3 {'ragged' if last < CV_TM else 'whole'} last tile", f"conv3x3 tiles {min(tiles, 2)}",
                    f"conv3x3 chunks {c['cin'] // 32}"}
    if kind == "q16":
        q, sc = launch_conv(run, c, "q16", xs, amax, scale)
        nhwc = launch_conv(run, c, "nhwc", xs, amax, scale)
        log.compare(f"conv3x3 nhwc | {name} | fp32 beside the int16 blocks", nhwc, r["ref"], r["A"], r["r32"])
        check_q16(run, c, key, q, sc, nhwc)
        deq = (q.float() * sc.unsqueeze(-1)).reshape(N, H, W, COUT).permute(0, 3, 1, 2)
        blockmax = nhwc.abs().reshape(N, 4, 64, H, W).amax(2, keepdim=True).expand(N, 4, 64, H, W).reshape(N, COUT, H, W)
        log.compare(f"conv3x3 q16 dequantised | {name} | out", deq, r["ref"], r["A"], r["r32"], R=torch.nan_to_num(blockmax.double()) * 2.0 ** -15)
        return
    out = launch_conv(run, c, kind, xs, amax, scale)
    log.compare(key + " | out", out, r["ref"], r["A"], r["r32"])
    if s.get("also_nhwc"):                               # "bit for bit the CV_OUT_NHWC result transposed" (conv3x3.hip, the modes' comment)
        nhwc = launch_conv(run, c, "nhwc", xs, amax, scale)
        require(image_equal(out.contiguous(), nhwc.contiguous()), f"{key}: not the bits of the channel-last result")
    if s.get("heads"):
        zero = out[:, 64:128]
        want = c["pmap"].t().reshape(1, COUT, H, W)[:, 64:128].expand_as(zero) if c["pmap"] is not None else torch.zeros_like(zero)
        require(bits_equal(zero.contiguous(), want.contiguous()), f"{key}: the all-zero head is not exactly {'the map' if c['pmap'] is not None else '0'}")
        for lo, hi, what in ((0, 64, "head x 1e-4"), (128, 256, "ordinary heads")):
            log.compare(f"{key} | {what}", out[:, lo:hi], r["ref"][:, lo:hi], r["A"][:, lo:hi], r["r32"][:, lo:hi])
    if "small_frame" in s:
        n = s["small_frame"]
        assert float(r["A"][n].max()) < 2.0 ** -9 * float(r["A"].max())
        log.compare(f"{key} | the frame x 2^-12", out[n], r["ref"][n], r["A"][n], r["r32"][n])
    if s.get("zero"):
        require(bits_equal(out.contiguous(), _addend(c, F32).expand_as(out).contiguous()), f"{key}: an all-zero image does not give the bias")
    if "pow2" in s:                                      # conv(2^k x) == 2^k conv(x), bit for bit (no bias)
        c1 = dict(c, x=c["x"] * 2.0 ** -s["pow2"], name=name + " unscaled")
        xs1 = run.dev(torch.zeros_like(r["xs"]))
        a1 = run.absmax([run.dev(c1["x"])], 0.0)
        run.pack("nchw", run.dev(c1["x"]), a1, xs1, 0)
        require(image_equal(run.host(xs1), r["xs"]), f"{key}: the image of 2^k x is not the image of x")
        base = launch_conv(run, c1, kind, xs1, a1, scale)
        require(bits_equal((base * 2.0 ** s["pow2"]).contiguous(), out.contiguous()), f"{key}: conv(2^k x) != 2^k conv(x)")
    return out


def check_conv_poison(log, name, run):
    """one NaN in one pixel and channel of one frame: NaN exactly on float64's footprint (3x3 pixels, every output channel, that
    frame), every clean element within the bound"""
    c, r = conv_case(name), conv_reference(name)
    n, _, h, w = c["poisoned"]
    nan = torch.isnan(r["ref"])
    fp = torch.zeros_like(nan)
    fp[n, :, max(h - 1, 0):h + 2, max(w - 1, 0):w + 2] = True
    assert torch.equal(nan, fp) and int(nan.sum()) == 9 * COUT, "float64's footprint is not the 3x3 window"
    check_conv(log, name, run)


# ------------------------------------------------------------------------------------------------ rac_conv3x3_temporal_fwd
TEMPORAL_CASES = {f"live{live} dead{cd} {H}x{W}{' q16' if q else ''}": dict(live=live, cin_dead=cd, H=H, W=W, q16=q)
                  for live, cd, (H, W), q in ((0, 32, (16, 16), False), (1, 64, (16, 32), False), (2, 32, (16, 32), True), (2, 64, (16, 16), False),
                                              (4, 64, (16, 16), True), (1, 32, (16, 16), True), (4, 32, (16, 32), False), (0, 64, (16, 16), True))}
TEMPORAL_CASES["poison live2 dead64 16x16"] = dict(live=2, cin_dead=64, H=16, W=16, q16=False, poison=True)
T_FRAMES, T_GROUPS, T_CIN = 4, 2, 128


@functools.lru_cache(maxsize=None)
def temporal_case(name):
    """Cin = 128 of which the channels from cin_dead on are, in the frames past a group's live ones, a per-channel constant"""
    s = TEMPORAL_CASES[name]
    live, cd, H, W = s["live"], s["cin_dead"], s["H"], s["W"]
    N, ch = T_FRAMES * T_GROUPS, T_CIN - cd
    g = torch.Generator().manual_seed(2000 + list(TEMPORAL_CASES).index(name))
    x = torch.randn(N, cd, H, W, generator=g)
    hv = torch.randn(T_GROUPS * live, ch, H, W, generator=g) * 0.5
    b_up = torch.randn(ch, generator=g) * 0.3
    weight = torch.randn(COUT, T_CIN, 3, 3, generator=g) * math.sqrt(2.0 / (9 * T_CIN))
    pmap = torch.randn(H * W, COUT, generator=g)
    if s.get("poison"):
        x[5, 7, H // 2, 3] = NAN                          # (live 2 of 4: frames 0, 1, 4, 5 are live) a live frame
        x[6, 9, 2, W // 2] = NAN                          # and a dead one
    ws, w_alpha = pack_conv3x3_weight(weight)
    floor = float(b_up.abs().max()) + (float(hv.abs().max()) if hv.numel() else 0.0)
    return dict(name=name, kind="nhwc", N=N, H=H, W=W, cin=T_CIN, cin_dead=cd, live=live, x=x, hv=hv, b_up=b_up, ws=ws, w_alpha=w_alpha, bias=None,
                pmap=pmap, cams=1, q16=s["q16"], floor=floor, spec=s)


@functools.lru_cache(maxsize=None)
def temporal_reference(name):
    c = temporal_case(name)
    N, H, W, cd = c["N"], c["H"], c["W"], c["cin_dead"]
    R0 = Restated()
    amax = R0.absmax([c["x"], c["hv"]], c["floor"])
    xs = torch.zeros(N, H + 2, W + 2, T_CIN // 32, 2, 32, dtype=F16)
    R0.pack("nchw", c["x"], amax, xs, 0)
    R0.pack("live", c["hv"], amax, xs, cd, c["b_up"], T_FRAMES, c["live"])
    X, Wv = image_values(xs, act_scale(float(amax))), unpack_conv3x3_weight(c["ws"], c["w_alpha"])
    add = c["pmap"].double().t().reshape(1, COUT, H, W)
    with torch.no_grad():
        ref = TF.conv2d(X, Wv) + add                     # the explicit image, dead frames included
        A = TF.conv2d(torch.nan_to_num(X.abs()), Wv.abs()) + add.abs()
        r32 = TF.conv2d(X.float(), Wv.float()) + add.float()
    # the fold: the constant the image holds in a dead frame's hidden half (the same in every dead frame and pixel), through the zero padding
    const = X[T_FRAMES - 1, cd:, 1, 1] if c["live"] < T_FRAMES else torch.zeros(T_CIN - cd, dtype=F64)
    dead_map = (c["pmap"].double() + dead_frame_bias_map(Wv[:, cd:], const, H, W)).float()
    return dict(xs=xs, amax=amax, ref=ref, A=A, r32=r32, dead_map=dead_map)


def check_temporal(log, name, run):
    c, r = temporal_case(name), temporal_reference(name)
    N, H, W, cd, live = c["N"], c["H"], c["W"], c["cin_dead"], c["live"]
    key = f"conv3x3 temporal{' q16' if c['q16'] else ''} | {name}"
    x, hv = run.dev(c["x"]), run.dev(c["hv"])
    amax = run.absmax([x, hv], c["floor"])
    require(bits_equal(run.host(amax).view(1), r["amax"].view(1)), f"{key}: amax")
    xs = run.dev(torch.zeros_like(r["xs"]))
    run.pack("nchw", x, amax, xs, 0)
    run.pack("live", hv, amax, xs, cd, run.dev(c["b_up"]), T_FRAMES, live)
    require(image_equal(run.host(xs), r["xs"]), f"{key}: the packed image differs from the restatement")
    temporal = (r["dead_map"], cd, T_FRAMES, live)
    is_live = torch.tensor([n % T_FRAMES < live for n in range(N)])
    log.reached |= {"conv3x3 temporal" + (" q16" if c["q16"] else ""), f"conv3x3 temporal live {live}"}
    plain = launch_conv(run, c, "nhwc", xs, amax, (1.0, 0.0))                     # rac_conv3x3_fwd on the explicit image
    if c["q16"]:
        q, sc = launch_conv(run, c, "q16", xs, amax, (1.0, 0.0), temporal=temporal)
        pq, psc = launch_conv(run, c, "q16", xs, amax, (1.0, 0.0))
        require(torch.equal(q[is_live], pq[is_live]) and image_equal(sc[is_live], psc[is_live]), f"{key}: live frames differ from rac_conv3x3_q16_fwd")
        out = (q.float() * sc.unsqueeze(-1)).reshape(N, H, W, COUT).permute(0, 3, 1, 2)
        blockmax = torch.nan_to_num(out.abs().double()).reshape(N, 4, 64, H, W).amax(2, keepdim=True).expand(N, 4, 64, H, W).reshape(N, COUT, H, W)
        log.compare(f"conv3x3 temporal q16 dequantised | {name} | out", out, r["ref"], r["A"], r["r32"], R=blockmax * (2.0 ** -15 * (1 + 2.0 ** -14)))
        return
    out = launch_conv(run, c, "nhwc", xs, amax, (1.0, 0.0), temporal=temporal)
    require(image_equal(out[is_live].contiguous(), plain[is_live].contiguous()), f"{key}: live frames differ from rac_conv3x3_fwd")
    log.compare(key + " | explicit image", plain, r["ref"], r["A"], r["r32"])
    log.compare(key + " | out", out, r["ref"], r["A"], r["r32"])
    if live < T_FRAMES:
        log.compare(key + " | dead frames", out[~is_live], r["ref"][~is_live], r["A"][~is_live], r["r32"][~is_live])


# ------------------------------------------------------------------------------------------------ conv3x3s2_c64_f16x3_kernel
S2_CASES = {"16x32 C32 out64": dict(H=16, W=32, N=3, cin=32, ctot=64), "16x32 C256 out96": dict(H=16, W=32, N=1, cin=256, ctot=96),
            "32x32 C256 out64": dict(H=32, W=32, N=1, cin=256, ctot=64), "32x32 C32 out96": dict(H=32, W=32, N=3, cin=32, ctot=96),
            "2x512 C32 out96": dict(H=2, W=512, N=2, cin=32, ctot=96), "2x512 C256 out64": dict(H=2, W=512, N=1, cin=256, ctot=64),
            "512x2 C256 out96": dict(H=512, W=2, N=1, cin=256, ctot=96), "512x2 C32 out64": dict(H=512, W=2, N=2, cin=32, ctot=64),
            "poison 16x32 C32": dict(H=16, W=32, N=3, cin=32, ctot=96, poison=True), "no bias 16x32": dict(H=16, W=32, N=1, cin=32, ctot=64, bias=False)}
S2_IMAGE_C = 320


@functools.lru_cache(maxsize=None)
def s2_case(name):
    s = S2_CASES[name]
    N, H, W, cin = s["N"], s["H"], s["W"], s["cin"]
    g = torch.Generator().manual_seed(3000 + list(S2_CASES).index(name))
    x = torch.randn(N, S2_IMAGE_C, H, W, generator=g)
    weight = torch.randn(64, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
    bias = torch.randn(64, generator=g) * 0.3 if s.get("bias", True) else None
    if s.get("poison"):
        x[1, 5, 7, 10] = NAN                              # an odd row and an even column: taps of 2 x 1 output pixels
        x[2, 40, 3, 3] = NAN                              # a channel the launch does not read
    ws, w_alpha = pack_conv3x3_weight(weight, cout=64)
    return dict(name=name, N=N, H=H, W=W, cin=cin, ctot=s["ctot"], x=x, ws=ws, w_alpha=w_alpha, bias=bias, spec=s)


@functools.lru_cache(maxsize=None)
def s2_reference(name):
    c = s2_case(name)
    N, H, W, cin = c["N"], c["H"], c["W"], c["cin"]
    amax = Restated().absmax([c["x"]], 0.0)
    xs = torch.zeros(N, H + 2, W + 2, S2_IMAGE_C // 32, 2, 32, dtype=F16)
    Restated().pack("nchw", c["x"], amax, xs, 0)
    X, Wv = image_values(xs, act_scale(float(amax)))[:, :cin], unpack_conv3x3_weight(c["ws"], c["w_alpha"])
    b = c["bias"] if c["bias"] is not None else torch.zeros(64)
    with torch.no_grad():
        ref = TF.conv2d(X, Wv, b.double(), stride=2)
        A = TF.conv2d(torch.nan_to_num(X.abs()), Wv.abs(), b.double().abs(), stride=2)
        r32 = TF.conv2d(X.float(), Wv.float(), b, stride=2)
    assert tuple(ref.shape) == (N, 64, H // 2, W // 2)
    return dict(xs=xs, amax=amax, ref=ref, A=A, r32=r32)


def check_s2(log, name, run):
    c, r = s2_case(name), s2_reference(name)
    N, H, W, cin, ctot = c["N"], c["H"], c["W"], c["cin"], c["ctot"]
    key = f"conv3x3s2 | {name}"
    assert (H // 2) * (W // 2) % S2_TM == 0
    log.reached |= {"conv3x3s2", f"conv3x3s2 tiles {min((H // 2) * (W // 2) // S2_TM, 2)}", f"conv3x3s2 chunks {cin // 32}"}
    x = run.dev(c["x"])
    amax = run.absmax([x], 0.0)
    xs = run.dev(torch.zeros_like(r["xs"]))
    run.pack("nchw", x, amax, xs, 0)
    require(image_equal(run.host(xs), r["xs"]), f"{key}: the packed image differs from the restatement")
    full, dst = guarded(run, N, (ctot, H // 2, W // 2))
    run.conv_s2(xs, run.dev(c["ws"]), c["w_alpha"], amax, run.dev(c["bias"]) if c["bias"] is not None else None, dst, N, H, W, cin, S2_IMAGE_C)
    out = taken(run, full, N)
    assert bool(torch.isnan(out[:, 64:]).all()), "conv_s2 wrote past its 64 channels"
    if c["spec"].get("poison"):
        assert int(torch.isnan(r["ref"]).sum()) == 2 * 64 and bool(torch.isnan(r["ref"][1, :, 3:5, 5]).all())
    log.compare(key + " | out", out[:, :64], r["ref"], r["A"], r["r32"])


# =============================================================================================== conv_direct_kernel
def _direct_cases():
    c = {}
    # stride-2 image: 2 / 3 / 8 chunks; 2x2 gives one output pixel, 12x20 a ragged tile of 60; frame maps of two groups, a nonzero first,
    # input and output maps that differ; in_chunk0 > 0; out_chunk0 > 0 in a wider image
    c["image s2 k2 2x2"] = dict(mode="image", stride=2, k=2, H=2, W=2, N=4, cout=64, in_frames=(2, 3, 1), out_frames=(2, 4, 1), in_chunk0=1,
                                in_total=4, out_chunk0=1, out_total=4)
    c["image s2 k3 12x20"] = dict(mode="image", stride=2, k=3, H=12, W=20, N=3, cout=64, in_total=3, out_total=2, bias=False)
    c["image s2 k8 16x16"] = dict(mode="image", stride=2, k=8, H=16, W=16, N=2, cout=128, in_total=10, out_chunk0=2, out_total=6,
                                  in_frames=(1, 2, 1), out_frames=(1, 1, 0))
    c["image s2 k2 8x8"] = dict(mode="image", stride=2, k=2, H=8, W=8, N=1, cout=64, in_total=2, out_total=2)
    # stride-1 image (256 pixels per workgroup): ragged 240, exactly one tile, 4 pixels
    c["image s1 12x20"] = dict(mode="image", stride=1, k=2, H=12, W=20, N=3, cout=64, in_total=2, out_total=2, in_frames=(3, 4, 1), out_frames=(1, 2, 0))
    c["image s1 16x16"] = dict(mode="image", stride=1, k=2, H=16, W=16, N=1, cout=128, in_chunk0=2, in_total=4, out_chunk0=1, out_total=6, bias=False)
    c["image s1 2x2"] = dict(mode="image", stride=1, k=2, H=2, W=2, N=2, cout=64, in_total=2, out_total=2)
    c["image_relu 12x20"] = dict(mode="image_relu", stride=1, k=2, H=12, W=20, N=2, cout=64, in_total=2, out_chunk0=2, out_total=4)
    c["image_relu 4x6"] = dict(mode="image_relu", stride=1, k=2, H=4, W=6, N=3, cout=128, in_total=3, in_chunk0=1, out_total=4,
                               in_frames=(1, 2, 1), out_frames=(3, 3, 2))
    c["image_relu 16x16"] = dict(mode="image_relu", stride=1, k=2, H=16, W=16, N=1, cout=64, in_total=2, out_total=2, bias=False)
    # f32 (128 pixels per workgroup): 1 / 2 / 4 chunks; the per-pixel map with and without bias
    c["f32 k1 4x6"] = dict(mode="f32", stride=1, k=1, H=4, W=6, N=3, cout=64, in_total=1)
    c["f32 k2 12x20 map bias"] = dict(mode="f32", stride=1, k=2, H=12, W=20, N=2, cout=192, in_total=4, in_chunk0=2, pmap=True, in_frames=(1, 2, 1))
    c["f32 k4 8x8 map"] = dict(mode="f32", stride=1, k=4, H=8, W=8, N=3, cout=128, in_total=4, pmap=True, bias=False)
    c["f32 k2 16x16"] = dict(mode="f32", stride=1, k=2, H=16, W=16, N=1, cout=64, in_total=2, bias=False)
    c["f32 k1 2x2 map"] = dict(mode="f32", stride=1, k=1, H=2, W=2, N=1, cout=64, in_total=2, in_chunk0=1, pmap=True)
    c["f32_cf_relu 12x20"] = dict(mode="f32_cf_relu", stride=1, k=2, H=12, W=20, N=2, cout=256, in_total=2)
    c["f32_cf_relu 2x2"] = dict(mode="f32_cf_relu", stride=1, k=2, H=2, W=2, N=3, cout=64, in_total=3, in_chunk0=1, bias=False, in_frames=(3, 3, 1))
    c["f32_cf_relu 8x8"] = dict(mode="f32_cf_relu", stride=1, k=2, H=8, W=8, N=1, cout=64, in_total=2)
    # the GRU: one step from h_prev = NULL (no convolution), one from a given h_prev
    c["gru k0 4x6"] = dict(mode="gru", stride=1, k=0, H=4, W=6, N=2, cout=192, in_total=2, out_total=2, steps=3, t=1)
    c["gru k0 12x20"] = dict(mode="gru", stride=1, k=0, H=12, W=20, N=1, cout=192, in_total=2, out_chunk0=1, out_total=4, steps=1, t=0)
    c["gru k2 12x20"] = dict(mode="gru", stride=1, k=2, H=12, W=20, N=2, cout=192, in_total=2, out_total=2, steps=3, t=1)
    c["gru k2 8x8"] = dict(mode="gru", stride=1, k=2, H=8, W=8, N=2, cout=192, in_total=2, out_total=2, steps=2, t=1)
    c["gru k2 2x2"] = dict(mode="gru", stride=1, k=2, H=2, W=2, N=1, cout=192, in_total=2, out_total=2, steps=4, t=3)
    for mode in ("image", "image_relu", "f32", "f32_cf_relu", "gru"):
        c[f"poison {mode}"] = dict(mode=mode, stride=1, k=2, H=12, W=20, N=3, cout=192 if mode == "gru" else 64, in_total=2, out_total=2, poison=True,
                                   **(dict(steps=2, t=1) if mode == "gru" else {}))
    c["poison image s2"] = dict(mode="image", stride=2, k=2, H=12, W=20, N=3, cout=64, in_total=2, out_total=2, poison=True)
    return c


DIRECT_CASES = _direct_cases()
DIRECT_PLAIN = [n for n, s in DIRECT_CASES.items() if not s.get("poison")]
DIRECT_POISON = [n for n, s in DIRECT_CASES.items() if s.get("poison")]


def host_image(values, bound, frames, total, chunk0, sentinel=True):
    """an activation image [frames, H+2, W+2, total, 2, 32] holding ``values`` {frame: [C,H,W]} in chunks chunk0.. at the scale of
    ``bound``; the other chunks hold the sentinel, the other frames zeros"""
    C, H, W = next(iter(values.values())).shape
    img = torch.zeros(frames, H + 2, W + 2, total, 2, 32, dtype=F16)
    if sentinel:
        keep = [k for k in range(total) if not chunk0 <= k < chunk0 + C // 32]
        img[:, :, :, keep] = SENTINEL
    for f, v in values.items():
        hi, lo = split_f16(v.float() * act_scale(bound))
        image_put(img[f:f + 1], hi[None], lo[None], chunk0)
    return img


@functools.lru_cache(maxsize=None)
def direct_case(name):
    """-> the keywords of one rac_conv_direct_fwd launch (host tensors) and what the checks need beside them"""
    s = DIRECT_CASES[name]
    mode, stride, k, H, W, N, cout = (s[x] for x in ("mode", "stride", "k", "H", "W", "N", "cout"))
    OH, OW = H // stride, W // stride
    g = torch.Generator().manual_seed(4000 + list(DIRECT_CASES).index(name))
    gru = mode == "gru"
    cin = 64 if gru else 32 * k
    kw = dict(N=N, H=H, W=W, in_chunks_total=s["in_total"], chunks=k, cout=cout, conv_stride=stride, in_chunk0=s.get("in_chunk0", 0))
    if gru:                                              # frames [N groups][steps], this launch is step t: h of step t - 1 -> h of step t
        steps, t = s["steps"], s["t"]
        fr_prev, fr_now = (1, steps, max(t - 1, 0)), (1, steps, t)
        kw.update(in_frames=fr_prev, out_frames=fr_now, xpart_frames=fr_now, h_prev_frames=fr_prev, h_out_frames=fr_now)
        in_frames, nframes_in = fr_prev, N * steps
    else:
        in_frames = s.get("in_frames", (1, 1, 0))
        kw.update(in_frames=in_frames)
        nframes_in = max(cd_frame(in_frames, n) for n in range(N)) + 2
    # the input image: signed normal values (the GRU: a state, |h| <= 1) at the scale of their bound
    x = torch.rand(N, cin, H, W, generator=g) * 2 - 1 if gru else torch.randn(N, cin, H, W, generator=g)
    if s.get("poison") and k:
        x[1, 9, H // 2, 3] = NAN
    amax = torch.tensor([float(torch.nan_to_num(x).abs().max())])
    in_scale = (None, 0.0, 1.0) if gru else (amax, 1.0, 0.0)
    in_bound = bound32(None if gru else float(amax), in_scale[1], in_scale[2])
    in_img = None
    if k:
        in_img = host_image({cd_frame(in_frames, n): x[n] for n in range(N)}, in_bound, nframes_in, s["in_total"], kw["in_chunk0"],
                            sentinel=not gru or s.get("out_chunk0", 0) > 0)
    weight = torch.randn(cout, cin, 3, 3, generator=g) * math.sqrt(2.0 / (9 * cin))
    ws, w_alpha = pack_conv3x3_weight(weight, cout=cout)
    bias = torch.randn(cout, generator=g) * 0.3 if s.get("bias", True) and not gru else None
    pmap = torch.randn(OH * OW, cout, generator=g) if s.get("pmap") else None
    kw.update(in_img=in_img if k else None, ws=ws if k else None, w_alpha=w_alpha, in_scale=in_scale, bias=bias, pixel_map=pmap)
    extra = dict(name=name, mode=mode, x=x, amax=amax, in_bound=in_bound, spec=s, OH=OH, OW=OW, cin=cin)
    if mode in ("image", "image_relu") or gru:
        out_frames = kw.get("out_frames") or s.get("out_frames", (1, 1, 0))
        if gru:
            out_scale, out_bound = (None, 0.0, 1.0), 1.0
        else:                                            # the bound the product derives: max row |W|_1 * amax + max |b|
            l1 = float(weight.abs().sum(dim=(1, 2, 3)).max())
            out_scale = (amax, l1, float(bias.abs().max()) if bias is not None else 0.0)
            out_bound = bound32(float(amax), out_scale[1], out_scale[2])
        nframes_out = max(cd_frame(out_frames, n) for n in range(N)) + 2
        kw.update(out_frames=out_frames, out_scale=out_scale, out_chunks_total=s["out_total"], out_chunk0=s.get("out_chunk0", 0))
        extra.update(out_bound=out_bound, nframes_out=nframes_out)
    if gru:
        xpart = torch.randn(N * steps, OH * OW, 192, generator=g) * 1.5
        h_prev = None
        if k:                                            # the state the image holds, as the previous step stored it: h_prev [frames, HW, 64]
            h_prev = torch.zeros(N * steps, OH * OW, 64)
            for n in range(N):
                h_prev[cd_frame(fr_prev, n)] = torch.nan_to_num(x[n]).reshape(64, OH * OW).t()
        kw.update(xpart=xpart, h_prev=h_prev)
        extra.update(nframes_out=N * steps, same_image=s.get("out_chunk0", 0) == 0)
    return kw, extra


def cd_operands(kw, fault=None):
    """-> (the input image's frames and chunks the launch reads [N,Hp,Wp,k,2,32], its scale)"""
    frames = [cd_frame(kw["in_frames"], n, fault) for n in range(kw["N"])]
    xs = kw["in_img"][frames][:, :, :, kw["in_chunk0"]:kw["in_chunk0"] + kw["chunks"]]
    am, mul, add = kw["in_scale"]
    return xs, act_scale(bound32(float(am) if am is not None else None, mul, add))


@functools.lru_cache(maxsize=None)
def direct_reference(name):
    """-> ref, A, r32 [N,Cout,OH,OW] of the convolution part (+ bias + map, ReLU applied); for the GRU: of h [N,64,OH,OW]"""
    kw, e = direct_case(name)
    N, cout, stride, OH, OW = kw["N"], kw["cout"], kw["conv_stride"], e["OH"], e["OW"]
    with torch.no_grad():
        if kw["chunks"]:
            xs, scale = cd_operands(kw)
            X, Wv = image_values(xs, scale), unpack_conv3x3_weight(kw["ws"], kw["w_alpha"])
            pre = TF.conv2d(X, Wv, stride=stride)
            A = TF.conv2d(torch.nan_to_num(X.abs()), Wv.abs(), stride=stride)
            p32 = TF.conv2d(X.float(), Wv.float(), stride=stride)
        else:
            pre = A = torch.zeros(N, cout, OH, OW, dtype=F64)
            p32 = torch.zeros(N, cout, OH, OW)
        if e["mode"] != "gru":
            for t in (kw["bias"].view(1, cout, 1, 1) if kw["bias"] is not None else None,
                      kw["pixel_map"].t().reshape(1, cout, OH, OW) if kw["pixel_map"] is not None else None):
                if t is not None:
                    pre, A, p32 = pre + t.double(), A + t.double().abs(), p32 + t
            if "relu" in e["mode"]:
                pre, p32 = torch.relu(pre), torch.relu(p32)
            return dict(ref=pre, A=A, r32=p32)
        xp = torch.stack([kw["xpart"][cd_frame(kw["xpart_frames"], n)] for n in range(N)]).permute(0, 2, 1).reshape(N, 192, OH, OW)
        hp = torch.zeros(N, 64, OH, OW)
        if kw["h_prev"] is not None:
            hp = torch.stack([kw["h_prev"][cd_frame(kw["h_prev_frames"], n)] for n in range(N)]).permute(0, 2, 1).reshape(N, 64, OH, OW)
        ref, Ah = gru_formula(pre + xp.double(), hp.double(), A + xp.double().abs())
        r32, _ = gru_formula(p32 + xp, hp)
    return dict(ref=ref, A=Ah, r32=r32)


def gru_formula(gates, hp, A_gates=None, fault=None):
    """models/racformer_transformer.py:714-720 on the gate pre-activations [N,192,..] and h_prev [N,64,..] -> (h, its magnitude):
    sigmoid' <= 1/4 and tanh' <= 1 times the pre-activations' A, and every intermediate's own size for its own rounding"""
    zg, rg, cg = gates.split(64, dim=1)
    z, r = torch.sigmoid(zg), torch.sigmoid(rg)
    s = cg + r * hp
    cand = torch.tanh(s)
    h = z * hp + (1 - z) * cand if fault == "gru_z_swapped" else (1 - z) * hp + z * cand
    if A_gates is None:
        return h, None
    Az, Ar, Ac = A_gates.split(64, dim=1)
    ah = hp.abs()
    A_z, A_r = Az / 4 + z, Ar / 4 + r
    A_cand = Ac + A_r * ah + 2 * (r * hp).abs() + s.abs() + cand.abs()
    A_h = A_z * ah + 2 * ((1 - z) * hp).abs() + A_z * cand.abs() + z * A_cand + 2 * (z * cand).abs()
    return h, torch.nan_to_num(A_h)


def image_R(ref, bound):
    """what an image gives away of a value y at the scale of ``bound``: 2^-22 |y| + 2^-25 / scale"""
    return 2.0 ** -22 * torch.nan_to_num(ref.double().abs()) + 2.0 ** -25 / act_scale(bound)


def check_direct(log, name, run):
    kw, e = direct_case(name)
    r = direct_reference(name)
    mode, N, cout, OH, OW = e["mode"], kw["N"], kw["cout"], e["OH"], e["OW"]
    inst, ppw = cd_instance(mode, kw["conv_stride"], kw["chunks"])
    npix = OH * OW
    log.reached |= {"direct " + inst, f"direct {'ragged' if npix % ppw else 'whole'} pixel tiles", f"direct pixel tiles {min((npix + ppw - 1) // ppw, 2)}"}
    key = f"direct {inst} | {name}"
    dv = lambda t: run.dev(t) if t is not None else None                        # noqa: E731
    scale_dev = lambda sc: (dv(sc[0]), sc[1], sc[2])                             # noqa: E731
    args = dict(kw, in_img=dv(kw["in_img"]), ws=dv(kw["ws"]), bias=dv(kw["bias"]), pixel_map=dv(kw["pixel_map"]), in_scale=scale_dev(kw["in_scale"]))
    if e["spec"].get("poison") and kw["chunks"]:
        nan = torch.isnan(r["ref"])
        assert 0 < int(nan.sum()) <= 9 * nan.shape[1] and bool(nan[1].any()) and not bool(nan[[0, 2]].any())
    if mode in ("f32", "f32_cf_relu"):
        rest = (npix, cout) if mode == "f32" else (cout, npix)
        full, dst = guarded(run, N, rest)
        run.conv_direct(mode, **args, out_f32=dst)
        out = taken(run, full, N)
        out = out.permute(0, 2, 1) if mode == "f32" else out
        log.compare(key + " | out", out.reshape(N, cout, OH, OW), r["ref"], r["A"], r["r32"])
        return
    # an image destination: zeros, the sentinel in the chunks this launch does not own; frames of the output map
    oc0, octot = kw["out_chunk0"], kw["out_chunks_total"]
    nch = (64 if mode == "gru" else cout) // 32
    if mode == "gru" and e["same_image"] and kw["in_img"] is not None:
        before = kw["in_img"].clone()                    # the product's arrangement: the state's image is read and written, other frames
    else:
        before = torch.zeros(e["nframes_out"], OH + 2, OW + 2, octot, 2, 32, dtype=F16)
        before[:, :, :, [k for k in range(octot) if not oc0 <= k < oc0 + nch]] = SENTINEL
    img = run.dev(before.clone())
    args.update(out_img=img, out_scale=scale_dev(kw["out_scale"]))
    if mode == "gru" and e["same_image"] and kw["in_img"] is not None:
        args["in_img"] = img
    h_full = None
    if mode == "gru":
        h_full, h_out = guarded(run, e["nframes_out"], (npix, 64), lead=1)
        args.update(xpart=dv(kw["xpart"]), h_prev=dv(kw["h_prev"]), h_out=h_out)
    run.conv_direct(mode, **args)
    got_img = run.host(img)
    frames = [cd_frame(kw["out_frames"], n) for n in range(N)]
    owned = torch.zeros(before.shape, dtype=torch.bool)
    owned[frames, 1:-1, 1:-1, oc0:oc0 + nch] = True
    same = got_img.view(torch.int16) == before.view(torch.int16)
    require(bool(same[~owned].all()), f"{key}: {int((~same[~owned]).sum())} half-words changed outside the destination (border, other chunks, other frames)")
    vals = image_values(got_img[frames][:, :, :, oc0:oc0 + nch], act_scale(e["out_bound"]))[:, :, 1:-1, 1:-1]
    if mode != "gru":
        log.compare(key + " | image", vals, r["ref"], r["A"], r["r32"], R=image_R(r["ref"], e["out_bound"]))
        return
    h_all = taken(run, h_full, e["nframes_out"], lead=1)
    rows = torch.zeros(e["nframes_out"], dtype=torch.bool)
    rows[frames] = True
    assert bool(torch.isnan(h_all[~rows]).all()), "the GRU wrote h_out frames outside its frame map"
    h = h_all[frames].permute(0, 2, 1).reshape(N, 64, OH, OW)
    log.compare(key + " | h_out", h, r["ref"], r["A"], r["r32"], lolo=kw["chunks"] > 0)
    ok = ~torch.isnan(h)
    require(bool((h[ok].abs() <= 1).all()), f"{key}: |h| > 1")
    require(torch.equal(torch.isnan(vals), ~ok), f"{key}: the image's NaN are not h_out's")
    bad = ok & ~((vals - h.double()).abs() <= image_R(h, 1.0))
    require(not bool(bad.any()), f"{key}: {int(bad.sum())} image values further than 2^-22 |y| + 2^-25 / scale from h_out")


# ------------------------------------------------------------------------------------------------ rac_upsample2x_image_fwd
UPSAMPLE_CASES = {"1x1": (2, 1, 1, 32, 1.0), "3x4": (3, 3, 4, 64, 1.0), "10x6": (3, 10, 6, 64, 1.0), "3x4 bound 5": (1, 3, 4, 32, 5.0)}


def check_upsample(log, name, run):
    frames, h, w, C, bound = UPSAMPLE_CASES[name]
    g = torch.Generator().manual_seed(5000 + list(UPSAMPLE_CASES).index(name))
    x = (torch.rand(frames, h, w, C, generator=g) * 2 - 1) * bound                  # channel-last
    before = torch.zeros(frames + 2, 2 * h + 2, 2 * w + 2, C // 32, 2, 32, dtype=F16)
    before[[0, -1]] = SENTINEL
    img = run.dev(before.clone())
    run.upsample_image(run.dev(x), img[1:-1], bound)
    got = run.host(img)
    owned = torch.zeros(before.shape, dtype=torch.bool)
    owned[1:-1, 1:-1, 1:-1] = True
    require(bool((got.view(torch.int16) == before.view(torch.int16))[~owned].all()), f"upsample2x_image {name}: border or neighbouring frames changed")
    vals = image_values(got[1:-1], act_scale(bound))[:, :, 1:-1, 1:-1]
    xc = x.permute(0, 3, 1, 2).contiguous()
    ref = upsample64(xc)
    A = upsample64(xc, magnitude=True) + upsample64(xc, position=True)
    r32 = TF.interpolate(xc, scale_factor=2, mode="bilinear", align_corners=True)
    log.reached.add("upsample2x_image")
    log.compare(f"upsample2x_image | {name} | image", vals, ref, A, r32, R=image_R(ref, bound), lolo=False)


# =============================================================================================== the restatement and its faults
FAULTS = ("tap_as_padding", "xlo_whi_dropped_in_chunk", "ragged_tile_shifted", "map_without_tile_offset", "dead_gets_live_map",
          "live_on_chunks_dead", "cam_group_swapped", "frame_unscaled_twice", "s2_centred_at_2o_plus_1", "frame_map_div_mod_swapped",
          "weight_chunks_exchanged", "gru_z_swapped", "relu_drops_nan")
# the case each control is run on (tests/test_conv_fwd_f64_cpu.py), as (check, case)
FAULT_CASES = {"tap_as_padding": ("conv", "nhwc bias 16x17"), "xlo_whi_dropped_in_chunk": ("conv", "nhwc bias 16x32 N3 C320"),
               "ragged_tile_shifted": ("conv", "nhwc bias 16x17"), "map_without_tile_offset": ("conv", "nhwc map 16x32"),
               "dead_gets_live_map": ("temporal", "live2 dead64 16x16"), "live_on_chunks_dead": ("temporal", "live2 dead64 16x16"),
               "cam_group_swapped": ("conv", "grouped cams3 9x29"), "frame_unscaled_twice": ("conv", "nhwc no bias 9x29"),
               "s2_centred_at_2o_plus_1": ("s2", "32x32 C32 out96"), "frame_map_div_mod_swapped": ("direct", "image s2 k2 2x2"),
               "weight_chunks_exchanged": ("direct", "f32 k2 16x16"), "gru_z_swapped": ("direct", "gru k2 8x8"),
               "relu_drops_nan": ("conv_poison", "poison nchw_relu")}


def relu(t, fault=None):
    y = torch.relu(t)
    return torch.where(torch.isnan(t), torch.zeros_like(t), y) if fault == "relu_drops_nan" else y


def core(xs, ws, stride=1, fault=None):
    """the kernels' accumulator: the three kept products of the half-words, each a float32 convolution, added in float32
    xs [N,Hp,Wp,k,2,32] f16, ws [9,k,cout,2,32] f16 -> [N,cout,OH,OW] f32 (still times both powers of two)"""
    xh, xl = image_halves(xs)
    wh, wl = weight_halves(ws)
    if fault == "weight_chunks_exchanged":
        perm = list(range(wh.shape[1]))
        perm[:64] = perm[32:64] + perm[:32]
        wh, wl = wh[:, perm], wl[:, perm]
    xl2 = xl
    if fault == "xlo_whi_dropped_in_chunk":
        xl2 = xl.clone()
        xl2[:, 96:128] = 0
    if fault == "s2_centred_at_2o_plus_1":
        xh, xl, xl2 = (TF.pad(t[:, :, 1:, 1:], (0, 1, 0, 1)) for t in (xh, xl, xl2))
    with torch.no_grad():
        acc = TF.conv2d(xh, wl, stride=stride) + TF.conv2d(xl2, wh, stride=stride) + TF.conv2d(xh, wh, stride=stride)
        if fault == "tap_as_padding":                    # column 0: the tap above (dy = 0, dx = 1) read as padding
            w1 = torch.zeros_like(wh)
            w1[:, :, 0, 1] = wh[:, :, 0, 1]
            acc[..., 0] -= TF.conv2d(xh, w1, stride=stride)[..., 0]
    return acc


class Restated:
    """the runner of the CPU module; ``fault``: one of FAULTS, the deliberately wrong variant of a negative control"""

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault

    def dev(self, t):
        return t

    def host(self, t):
        return t

    def absmax(self, srcs, floor):
        m = torch.tensor(float(floor), dtype=F32)
        for s in srcs:
            if s.numel():
                a = s.float().abs()
                m = torch.maximum(m, torch.where(torch.isnan(a), torch.zeros_like(a), a).max())
        return m.view(1)

    def pack(self, kind, src, amax, xs, c_offset, bias=None, T=1, live=1):
        scale = act_scale(float(amax))
        if kind == "cl":
            v = src.permute(0, 3, 1, 2)
        elif kind == "live":
            N, G = xs.shape[0], xs.shape[0] // T
            C, H, W = src.shape[1:]
            v = torch.zeros(G, T, C, H, W)
            v[:, :live] = src.view(G, live, C, H, W)
            v = v.view(N, C, H, W)
            if bias is not None:
                v = v + bias.view(1, C, 1, 1)
        else:
            v = src
        hi, lo = split_f16(v.float() * scale)
        image_put(xs, hi, lo, c_offset // 32)

    def quantize(self, value):
        return quantize_host(value)

    def conv(self, kind, xs, ws, w_alpha, amax, dst, N, H, W, cin, bias=None, pmap=None, cams=1, scale=(1.0, 0.0), temporal=None):
        f = self.fault
        HW = H * W
        if kind == "nchw_relu":
            sc = act_scale(bound32(float(amax) if amax is not None else None, scale[0], scale[1]))
        else:
            sc = act_scale(float(amax))
        unscale = torch.tensor(w_alpha / sc, dtype=F32)
        v = core(xs, ws, fault=f) * unscale
        if f == "frame_unscaled_twice":
            v[1] = v[1] * 0.5
        add = torch.zeros(N, COUT, H, W)
        if pmap is not None:
            m = pmap
            if f == "map_without_tile_offset":
                m = pmap[torch.arange(HW) % CV_TM]
            add = add + m.t().reshape(1, COUT, H, W)
        elif bias is not None:
            add = add + bias.view(1, COUT, 1, 1)
        if temporal is not None:
            pd, cin_dead, T, live = temporal
            dead = torch.tensor([n % T >= live for n in range(N)])
            if f == "live_on_chunks_dead":
                dead[0] = True
            if bool(dead.any()):
                kd = cin_dead // 32
                v[dead] = core(xs[dead][:, :, :, :kd], ws[:, :kd], fault=f) * unscale
                if f == "live_on_chunks_dead":
                    dead[0] = False
                if f != "dead_gets_live_map":
                    add[dead] = pd.t().reshape(1, COUT, H, W)
        v = v + add
        if kind == "nchw_relu":
            v = relu(v, f)
        if f == "ragged_tile_shifted":                   # the last tile's rows take the pixel after theirs
            tiles, last = conv_tiles(H, W)
            flat = v.reshape(N, COUT, HW)
            s0 = (tiles - 1) * CV_TM
            flat[:, :, s0:] = flat[:, :, torch.arange(s0 + 1, HW + 1).clamp(max=HW - 1)].clone()
            v = flat.reshape(N, COUT, H, W)
        if kind == "q16":
            q, s = quantize_host(v.permute(0, 2, 3, 1).reshape(N, HW, 4, 64).contiguous())
            dst[0].copy_(q)
            dst[1].copy_(s)
        elif kind == "nhwc":
            dst.copy_(v.permute(0, 2, 3, 1))
        elif kind in ("nchw", "nchw_relu"):
            dst.copy_(v.reshape(N, COUT, HW))
        else:
            g = v.reshape(N // cams, cams, 4, 64, HW).permute(0, 2, 1, 4, 3)           # [bt, g, cam, HW, 64]
            if f == "cam_group_swapped":
                g = g.permute(0, 2, 1, 3, 4)
            dst.copy_(g.reshape(dst.shape))

    def conv_s2(self, xs, ws, w_alpha, amax, bias, dst, N, H, W, cin, cin_image):
        v = core(xs[:, :, :, :cin // 32], ws, stride=2, fault=self.fault) * torch.tensor(w_alpha / act_scale(float(amax)), dtype=F32)
        if bias is not None:
            v = v + bias.view(1, 64, 1, 1)
        dst[:, :64].copy_(v)

    def conv_direct(self, mode, N, H, W, in_img, in_chunks_total, chunks, ws, w_alpha, cout, in_scale, conv_stride=1, in_chunk0=0,
                    in_frames=(1, 1, 0), bias=None, out_img=None, out_chunks_total=0, out_chunk0=0, out_frames=(1, 1, 0), out_scale=None,
                    out_f32=None, pixel_map=None, xpart=None, xpart_frames=(1, 1, 0), h_prev=None, h_prev_frames=(1, 1, 0), h_out=None,
                    h_out_frames=(1, 1, 0)):
        f = self.fault
        assert cd_instance(mode, conv_stride, chunks) is not None, "rac_conv_direct_fwd refuses this launch"
        OH, OW = H // conv_stride, W // conv_stride
        if chunks:
            kw = dict(N=N, in_img=in_img, in_frames=in_frames, in_chunk0=in_chunk0, chunks=chunks, in_scale=in_scale)
            xs, sc = cd_operands(kw, f)
            v = core(xs, ws, stride=conv_stride, fault=f) * torch.tensor(w_alpha / sc, dtype=F32)
        else:
            v = torch.zeros(N, cout, OH, OW)
        so = 1.0
        if out_scale is not None:
            so = act_scale(bound32(float(out_scale[0]) if out_scale[0] is not None else None, out_scale[1], out_scale[2]))
        if mode == "gru":
            xp = torch.stack([xpart[cd_frame(xpart_frames, n)] for n in range(N)]).permute(0, 2, 1).reshape(N, 192, OH, OW)
            hp = torch.zeros(N, 64, OH, OW)
            if h_prev is not None:
                hp = torch.stack([h_prev[cd_frame(h_prev_frames, n)] for n in range(N)]).permute(0, 2, 1).reshape(N, 64, OH, OW)
            v, _ = gru_formula(v + xp, hp, fault=f)
            for n in range(N):
                h_out[cd_frame(h_out_frames, n)] = v[n].reshape(64, OH * OW).t()
        else:
            add = torch.zeros(1, cout, OH, OW)
            if bias is not None:
                add = add + bias.view(1, cout, 1, 1)
            if pixel_map is not None:
                add = add + pixel_map.t().reshape(1, cout, OH, OW)
            v = v + add
            if "relu" in mode:
                v = relu(v, f)
        if mode == "f32":
            out_f32.copy_(v.reshape(N, cout, OH * OW).permute(0, 2, 1))
        elif mode == "f32_cf_relu":
            out_f32.copy_(v.reshape(N, cout, OH * OW))
        else:
            hi, lo = split_f16(v * so)
            for n in range(N):
                fr = cd_frame(out_frames, n)              # (the frame-map control is on the input map alone: on both, the two swaps cancel)
                image_put(out_img[fr:fr + 1], hi[n:n + 1], lo[n:n + 1], out_chunk0)

    def upsample_image(self, src, img, bound):
        v = TF.interpolate(src.permute(0, 3, 1, 2).contiguous(), scale_factor=2, mode="bilinear", align_corners=True)
        hi, lo = split_f16(v * act_scale(bound))
        image_put(img, hi, lo, 0)


CHECKS = {"conv": check_conv, "conv_poison": check_conv_poison, "temporal": check_temporal, "s2": check_s2, "direct": check_direct}

# what a whole session has to reach (asserted by both modules once every case has run)
REACH = {f"conv3x3 {k}" for k in CONV_KINDS} | {"conv3x3 ragged last tile", "conv3x3 whole last tile", "conv3x3 tiles 1", "conv3x3 tiles 2",
                                                 "conv3x3 chunks 1", "conv3x3 chunks 3", "conv3x3 chunks 10", "conv3x3 temporal", "conv3x3 temporal q16",
                                                 "conv3x3s2", "conv3x3s2 tiles 1", "conv3x3s2 tiles 2", "conv3x3s2 chunks 1", "conv3x3s2 chunks 8",
                                                 "direct ragged pixel tiles", "direct whole pixel tiles", "direct pixel tiles 1", "direct pixel tiles 2",
                                                 "upsample2x_image"} \
    | {f"conv3x3 temporal live {k}" for k in (0, 1, 2, 4)} | {"direct " + k for k in CD_INSTANCES}
