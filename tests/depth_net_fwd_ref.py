"""The float64 criterion for DepthNet's forward kernels (csrc/depth_net.hip: cs_pack_kernel, cs_conv_kernel, dn_gates_kernel,
dn_pool_bias_kernel): cases, references, magnitudes, the restatement, its negative controls and the launchers' rules, shared by
tests/test_depth_net_fwd_f64_cpu.py and tests/test_depth_net_fwd_f64_gpu.py (test helper, no GPU).

The thing under test is a ``runner``: an object with
  dev(t) / host(t)                                   a CPU tensor onto the runner's device and back
  pack_rows(src, dst, c_off, c_pad, BN=None) -> rc   src [BN,C,hw,1] channel-first into the rows dst [BN,hw,ld]   (rac_conv_small_pack_fwd)
  conv_small(x, w, cout, H, W, ..., BN=None) -> rc   racformer_amd.depth_net.conv_small's keywords, ``out`` given     (rac_conv_small_fwd)
  gates(mlp, params, out, BN, C, branches)           out [branches,BN,C]                                              (rac_depthnet_gates_fwd)
  pool_bias(x, wp, bp, wb, out, BN, hw, ld, C, Cout) out [BN,Cout]                                                    (rac_depthnet_pool_bias_fwd)
(``BN=0``: the launch is made with BN = 0 on the given buffers and has to return 0 with nothing written.)
``Restated`` is the runner of the CPU module, the kernels' arithmetic in float32 torch: the live taps in ascending order, each 32
input channels of a tap one fma chain from zero (the product exact, one rounding a step), the chains added in float32 in ascending
order, the epilogue in the kernel's order; the vector kernels' fma chains and pixel segments likewise.  With ``fault=`` it is each
of the negative controls (FAULTS).

Stage A, cs_pack_kernel, bit for bit: the whole destination -- the written channels (a -0.0, a NaN and a subnormal among them), the
+0 padding behind them, and the sentinel everywhere else -- equals the restatement's.

Stage B, cs_conv_kernel, every output element:
    |got - ref| <= max(4 E_ref, 1) 2^-24 A
ref: F.conv2d in float64 (padding = dilation) of the float32 operands, the input x.double() * gate.double() on the gated channels,
the epilogue terms added in float64, then the ReLU (1-Lipschitz: the bound passes through).  A = conv(|gate x|, |w|) + |bias| +
|img_bias| + |bins row| + |cls row| + |residual|.  E_ref: the worst err / A, in 2^-24, of torch's float32 conv2d on the CPU with the
same epilogue in float32.  No lo x lo term: the kernel rounds no operand below fp32.  An element with A == 0 is exactly 0; NaN
exactly where float64 has NaN; no element is left out.  Every destination is a frame range and a channel range of a larger
NaN-filled buffer whose remainder must still be NaN, in both layouts; the input channels a launch does not read (ld_in > Cin) are
NaN and the weight columns >= Cout hold 3e30.

Stage C.  Gates: float64 of the header's formula; the magnitude of the last pre-activation s carried through the three layers,
A_0 = |x|, A_l = |W_l|^T A_(l-1) + |b_l| + |s_l| (what the layer's input may be off by, times the weights; the layer's own sum; its
own size for its own rounding; ReLU' <= 1);
    |got - ref| <= max(4 E_ref, 1) 2^-24 A_s / 4 + 2^-22 |ref|
(sigmoid' <= 1/4; 2^-22 |ref|: expf within 1 ulp, the addition and the correctly rounded division).  Pool bias: A_m = mean |x|,
A_y = |Wp|^T A_m + |bp|, A = |Wb|^T A_y, the stage B rule.  E_ref from the same formulas in float32 torch on the CPU."""
import functools
import math

import torch
import torch.nn.functional as TF

from conv_fwd_ref import RATIO, Log, guarded, image_equal, require, taken  # noqa: F401  (RATIO: written into the profile)
from rowwise_ref import F32, F64, NAN, OutOfBound, bits_equal  # noqa: F401  (OutOfBound: what the modules catch)

CS_TM, CS_TN, CS_TK = 64, 64, 32
DN_THREADS = 1024
PACK_SENTINEL = -7.25
UNREAD_W = 3.0e30                    # the weight columns >= Cout: large and finite, never zeros
N_BINS, N_CLS = 7, 5


# ------------------------------------------------------------------------------------------- the launchers' rules, restated
def conv_tiles(H, W):
    """cs_conv_kernel: (tiles of 64 pixels per image, valid pixels of the last one)"""
    t = (H * W + CS_TM - 1) // CS_TM
    return t, H * W - (t - 1) * CS_TM


def tap_offset(tp, ksize, dil):
    return ((tp // 3 - 1) * dil, (tp % 3 - 1) * dil) if ksize == 3 else (0, 0)


def live_taps(H, W, ksize, dil, fault=None):
    """the taps cs_conv_kernel stages: abs(dy) < H && abs(dx) < W, ascending; tap 0 alone for a 1x1"""
    if ksize == 1:
        return (0,)
    out = []
    for tp in range(9):
        dy, dx = tap_offset(tp, 3, dil)
        if (abs(dy) <= H and abs(dx) <= W) if fault == "dead_tap_le" else (abs(dy) < H and abs(dx) < W):
            out.append(tp)
    return tuple(out)


TAP_SETS = {(0,): "1x1", (4,): "centre only", (1, 4, 7): "column of taps (columns dead)", (3, 4, 5): "row of taps (rows dead)",
            tuple(range(9)): "all nine"}


def cout_class(cout):
    """(channel tiles, what the last tile holds)"""
    tiles, last = (cout + CS_TN - 1) // CS_TN, (cout - 1) % CS_TN + 1
    what = "single lane" if last == 1 else "inside the first wave column" if last <= 32 else "one channel in the second wave column" \
        if last == 33 else "half a tile" if last < 64 else "whole"
    return f"{tiles} tile{'s' if tiles > 1 else ''}, last {what}"


def pool_segments(hw, C):
    """dn_pool_bias_kernel: G = 1024 / C and the pixel range of each segment"""
    G = DN_THREADS // C
    return G, [(hw * g // G, hw * (g + 1) // G) for g in range(G)]


def gates_block(C):
    """floats of one branch's parameter block"""
    return 10 * C + 3 * (C * C + C)


# ------------------------------------------------------------------------------------------------------------- arithmetic
def fma_chain(a, b, start):
    """s = fma(a[..., k], b[..., k, :], s) for k ascending, in float32: a [..., P, K], b [..., K, N], start [..., P, N]
    (the product is exact in float64; the sum is rounded to float64, then to float32)"""
    s = start
    for k in range(a.shape[-1]):
        s = (a[..., k:k + 1].double() * b[..., k:k + 1, :].double() + s.double()).float()
    return s


def shifted(x, dy, dx, zero=True):
    """x [BN,H,W,C] -> the value at (h + dy, w + dx), a pixel outside the map read at its clamped address and zeroed by a select"""
    H, W = x.shape[1:3]
    hh, ww = torch.arange(H) + dy, torch.arange(W) + dx
    v = x[:, hh.clamp(0, H - 1)][:, :, ww.clamp(0, W - 1)]
    if zero:
        ok = ((hh >= 0) & (hh < H)).view(1, H, 1, 1) & ((ww >= 0) & (ww < W)).view(1, 1, W, 1)
        v = torch.where(ok, v, torch.zeros((), dtype=v.dtype))
    return v


def relu(t, fault=None):
    y = torch.relu(t)
    return torch.where(torch.isnan(t), torch.zeros_like(t), y) if fault == "relu_drops_nan" else y


def epilogue(acc, e, dtype=F32, fault=None, ld_out=None, magnitude=False):
    """acc [BN,hw,Cout] -> the kernel's epilogue in its order, in ``dtype``; ``magnitude``: the sum of the terms' absolute values"""
    BN, hw, cout = acc.shape
    ab = (lambda t: t.abs()) if magnitude else (lambda t: t)
    v = acc.to(dtype)
    if e.get("bias") is not None:
        v = v + ab(e["bias"].to(dtype)).view(1, 1, cout)
    if e.get("img_bias") is not None:
        v = v + ab(e["img_bias"].to(dtype)).view(BN, 1, cout)
    if e.get("bins") is not None:
        b, table = e["bins"].reshape(BN, hw).long(), e["bins_table"].to(dtype)
        ok = (b >= 0) & ((b <= N_BINS) if fault == "bins_row_for_n_bins" else (b < N_BINS))
        rows = ab(table[(b % N_BINS).clamp(0, N_BINS - 1)])
        v = v + torch.where(ok.unsqueeze(-1), rows, torch.zeros((), dtype=dtype))
    if e.get("cls") is not None:
        k, table = e["cls"].reshape(BN, hw).long(), e["cls_table"].to(dtype)
        ok = (k >= 0) & (k < N_CLS)
        row = torch.where(ok, k + (0 if fault == "cls_without_plus_1" else 1), torch.zeros_like(k))
        add = ab(table[row])
        if fault == "cls_out_of_range_adds_nothing":
            add = torch.where(ok.unsqueeze(-1), add, torch.zeros((), dtype=dtype))
        v = v + add
    res = None
    if e.get("residual") is not None:
        r = e["residual"]
        if fault == "residual_ld_out":
            idx = (torch.arange(BN * hw).view(-1, 1) * ld_out + torch.arange(cout).view(1, -1)).clamp(max=r.numel() - 1)
            res = r.reshape(-1)[idx].view(BN, hw, cout)
        else:
            res = r[:, :, :cout]
        res = ab(res.to(dtype))
    if magnitude:
        return v + (torch.nan_to_num(res) if res is not None else 0)
    if fault == "relu_before_residual" and e.get("relu"):
        return relu(v) + (res if res is not None else 0)
    if res is not None:
        v = v + res
    return relu(v, fault) if e.get("relu") else v


# =============================================================================================== stage A: cs_pack_kernel
# (C, hw, BN, c_off, c_pad, ld): every C, hw, BN, c_off and c_pad of the issue in at least one launch; the module's own pair of
# launches into rows of 320 (25 one-hot channels at 256, 32 embedding channels at 281 + 7 of padding: 313 -> 320)
PACK_CASES = {"C1 hw1": (1, 1, 1, 0, 0, None), "C31 hw31": (31, 31, 3, 0, 7, None), "C32 hw32": (32, 32, 1, 256, 0, None),
              "C33 hw33": (33, 33, 3, 256, 7, None), "C129 hw77": (129, 77, 1, 0, 7, None), "C33 hw704": (33, 704, 3, 0, 0, None),
              "C1 hw77 pad7": (1, 77, 3, 256, 7, None), "module 25 at 256": (25, 704, 1, 256, 0, 320), "module 32 at 281 pad 7": (32, 704, 1, 281, 7, 320)}


def check_pack(run, name, BN0=False):
    C, hw, BN, c_off, c_pad, ld = PACK_CASES[name]
    ld = ld or c_off + C + c_pad + 3
    g = torch.Generator().manual_seed(7000 + list(PACK_CASES).index(name))
    src = torch.randn(BN, C, hw, 1, generator=g)
    flat = src.view(-1)
    for i, v in enumerate((-0.0, NAN, 1.0e-41)):                 # a -0.0, a NaN and a subnormal among the values
        flat[(i * 37 + 5) % flat.numel() if flat.numel() > 3 else i % flat.numel()] = v
    full, dst = guarded(run, BN, (hw, ld), fill=PACK_SENTINEL)
    want = torch.full((BN, hw, ld), PACK_SENTINEL)
    if BN0:
        require(run.pack_rows(run.dev(src), dst, c_off, c_pad, BN=0) == 0, f"pack {name}: BN = 0 does not return 0")
    else:
        require(run.pack_rows(run.dev(src), dst, c_off, c_pad) == 0, f"pack {name}: rc")
        Restated().pack_rows(src, want, c_off, c_pad)
    got = taken(run, full, BN, fill=PACK_SENTINEL)
    bad = got.view(torch.int32) != want.view(torch.int32)
    require(not bool(bad.any()), f"pack {name}{' BN = 0' if BN0 else ''}: {int(bad.sum())} words differ ({int(bad[:, :, c_off:c_off + C].sum())} in the "
                                 f"written channels, {int(bad[:, :, c_off + C:c_off + C + c_pad].sum())} in the padding)")
    return (hw + 31) // 32, (C + c_pad + 31) // 32


# =============================================================================================== stage B: cs_conv_kernel
ALL_PARTS = ("bias", "img_bias", "bins", "cls", "residual", "relu")


def _case(H, W, BN, cin, cout, k=3, dil=1, parts=(), **kw):
    return dict(H=H, W=W, BN=BN, cin=cin, cout=cout, ksize=k, dil=dil, parts=tuple(parts), **kw)


def _conv_cases():
    c = {}
    # the maps: centre tap only at any dilation; less than a tile; exactly one; two with 13 pixels in the second
    c["1x1 map d1"] = _case(1, 1, 3, 32, 33, parts=("bias",), taps=(4,))
    c["1x1 map d6"] = _case(1, 1, 3, 96, 1, dil=6, taps=(4,))
    c["3x5 k1 channel-first"] = _case(3, 5, 1, 32, 24, k=1, parts=("bias", "relu"), layout="cf", c_off=3)
    c["3x5 d1 256->256 everything"] = _case(3, 5, 1, 256, 256, parts=ALL_PARTS, gate="all", taps=tuple(range(9)))
    c["3x5 d6"] = _case(3, 5, 1, 96, 64, dil=6, parts=("bias",), taps=(4,))
    c["8x8 d1 96->96 gate 32 everything"] = _case(8, 8, 2, 96, 96, parts=ALL_PARTS, gate="some", c_off=32)
    c["8x8 d1 256->256"] = _case(8, 8, 2, 256, 256, parts=("bias", "relu"))
    c["8x8 d1 256->256 residual"] = _case(8, 8, 2, 256, 256, parts=("bias", "residual", "relu"))
    c["7x11 d1 256->64 ld_in"] = _case(7, 11, 2, 256, 64, parts=("bias", "relu"), ld_in_extra=8)
    c["7x11 k1 1024->64"] = _case(7, 11, 2, 1024, 64, k=1, parts=("bias", "img_bias", "relu"))
    c["7x11 k1 1024->33 channel-first"] = _case(7, 11, 2, 1024, 33, k=1, parts=("bias",), layout="cf", c_off=24)
    # rows live with columns dead, the transpose, and a dilation that equals the height (the tap at |dy| = H is dead)
    c["8x5 d6"] = _case(8, 5, 2, 96, 33, dil=6, parts=("bias", "relu"), taps=(1, 4, 7))
    c["5x8 d6"] = _case(5, 8, 2, 32, 64, dil=6, parts=("bias",), taps=(3, 4, 5), layout="cf")
    c["6x7 d6"] = _case(6, 7, 1, 32, 24, dil=6, taps=(3, 4, 5))
    c["8x5 d6 256->96"] = _case(8, 5, 2, 256, 96, dil=6, parts=("bias", "relu"), taps=(1, 4, 7))
    # ASPP's map and dilations (11 whole tiles; rows dead at 18), written into wider rows at a channel offset, and 20 x 23 x 3
    for i, dil in enumerate((1, 6, 12, 18)):
        c[f"16x44 d{dil}"] = _case(16, 44, 2, (96, 32, 96, 32)[i], (64, 96, 24, 33)[i], dil=dil, parts=("bias", "relu"), c_off=64 * i,
                                   taps=(3, 4, 5) if dil == 18 else tuple(range(9)))
        c[f"20x23 d{dil}"] = _case(20, 23, 3, (32, 96, 32, 96)[i], (33, 24, 96, 1)[i], dil=dil, parts=("bias",) if i % 2 else ("bias", "relu"),
                                   layout="cf" if i == 2 else "cl", taps=tuple(range(9)))
    # every epilogue part alone
    for p in ALL_PARTS:
        c[f"7x11 k1 {p} alone"] = _case(7, 11, 2, 32, 33, k=1, parts=(p,))
    c["7x11 d1 no epilogue"] = _case(7, 11, 2, 96, 24)
    c["7x11 k1 everything channel-first"] = _case(7, 11, 2, 96, 33, k=1, parts=ALL_PARTS, gate="all", layout="cf", c_off=5)
    # gates: all channels (one value exactly 0), 32 of 96
    c["7x11 k1 gate all"] = _case(7, 11, 2, 96, 64, k=1, parts=("bias",), gate="all")
    c["7x11 d1 gate 32 of 96"] = _case(7, 11, 2, 96, 33, parts=("bias",), gate="some")
    # magnitudes
    c["8x8 one image x 2^-12"] = _case(8, 8, 3, 256, 64, small_image=1)
    c["7x11 k1 one image x 2^-12 gated"] = _case(7, 11, 3, 96, 24, k=1, gate="all", small_image=2)
    for k in (20, -30):
        c[f"pow2 k{k}"] = _case(7, 11, 2, 96, 33, pow2=k)
    c["zero input"] = _case(7, 11, 2, 96, 33, parts=ALL_PARTS, gate="all", zero="input")
    c["zero input channel-first no relu"] = _case(3, 5, 1, 32, 24, parts=ALL_PARTS[:-1], zero="input", layout="cf")
    c["zero weight"] = _case(7, 11, 2, 96, 33, parts=ALL_PARTS, zero="weight")
    # poison
    for r in ((), ("relu",)):
        t = " relu" if r else ""
        c[f"poison input 20x23 d6{t}"] = _case(20, 23, 3, 32, 33, dil=6, parts=("bias",) + r, poison="input")
        c[f"poison input 16x44 d18{t}"] = _case(16, 44, 2, 32, 24, dil=18, parts=("bias",) + r, poison="input", layout="cf" if r else "cl")
        c[f"poison gate{t}"] = _case(7, 11, 3, 96, 33, k=1, parts=("bias",) + r, gate="some", poison="gate")
        for what, need in (("residual", ("residual",)), ("img_bias", ("img_bias",)), ("bins_row", ("bins",)), ("cls_row", ("cls",))):
            c[f"poison {what}{t}"] = _case(7, 11, 3, 32, 33, k=1, parts=("bias",) + need + r, poison=what)
    return c


CONV_CASES = _conv_cases()
CONV_PLAIN = [n for n, s in CONV_CASES.items() if not s.get("poison")]
CONV_POISON = [n for n, s in CONV_CASES.items() if s.get("poison")]
POISON_IMAGE = 1


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """-> the host operands of one rac_conv_small_fwd launch"""
    s = CONV_CASES[name]
    H, W, BN, cin, cout, k = s["H"], s["W"], s["BN"], s["cin"], s["cout"], s["ksize"]
    hw, parts = H * W, s["parts"]
    g = torch.Generator().manual_seed(6000 + list(CONV_CASES).index(name))
    ld_in = cin + s.get("ld_in_extra", 0)
    x = torch.full((BN, hw, ld_in), NAN)
    x[:, :, :cin] = torch.randn(BN, hw, cin, generator=g)
    ld_w = (cout + CS_TN - 1) // CS_TN * CS_TN
    w = torch.full((k * k, cin, ld_w), UNREAD_W)
    w[:, :, :cout] = torch.randn(k * k, cin, cout, generator=g) * math.sqrt(2.0 / (k * k * cin))
    e = dict(relu="relu" in parts)
    if "bias" in parts:
        e["bias"] = torch.randn(cout, generator=g) * 0.3
    if "img_bias" in parts:
        e["img_bias"] = torch.randn(BN, cout, generator=g) * 0.5            # (differs per image)
    if "bins" in parts:
        b = torch.randint(0, N_BINS, (BN, H, W), generator=g, dtype=torch.int32)
        b.view(-1)[:5] = torch.tensor([-1, 0, N_BINS - 1, N_BINS, 2 ** 30], dtype=torch.int32)
        e["bins"], e["bins_table"] = b, torch.randn(N_BINS, cout, generator=g)
    if "cls" in parts:
        q = torch.randint(0, N_CLS, (BN, H, W), generator=g, dtype=torch.int32)
        q.view(-1)[-5:] = torch.tensor([-2, -1, 0, N_CLS - 1, N_CLS], dtype=torch.int32)
        e["cls"], e["cls_table"] = q, torch.randn(N_CLS + 1, cout, generator=g)
    if "residual" in parts:
        r = torch.full((BN, hw, cout + 5), NAN)                             # ld_res > Cout, the columns behind unread
        r[:, :, :cout] = torch.randn(BN, hw, cout, generator=g)
        e["residual"] = r
    gate = None
    if s.get("gate"):
        gate = torch.rand(BN, cin if s["gate"] == "all" else 32, generator=g)   # (sigmoid's range; differs per image)
        gate[0, 5] = 0.0
    if "small_image" in s:
        x[s["small_image"]] *= 2.0 ** -12
    if "pow2" in s:
        x = x * 2.0 ** s["pow2"]
    if s.get("zero") == "input":
        x[:, :, :cin] = 0
    if s.get("zero") == "weight":
        w[:, :, :cout] = 0
    where = None
    if s.get("poison"):
        n, what = POISON_IMAGE, s["poison"]
        if what == "input":
            where = (n, (H // 2) * W + W // 2, 17)
            x[where] = NAN
        elif what == "gate":
            gate[n, 9] = NAN
        elif what == "residual":
            where = (n, hw // 3, 7)
            e["residual"][where] = NAN
        elif what == "img_bias":
            where = (n, 11)
            e["img_bias"][where] = NAN
        elif what == "bins_row":
            e["bins_table"][3] = NAN
        else:
            e["cls_table"][0, 4] = NAN                                       # row 0: the classes outside 0 .. n_cls - 1
    layout, c_off = s.get("layout", "cl"), s.get("c_off", 0)
    return dict(name=name, spec=s, H=H, W=W, BN=BN, hw=hw, cin=cin, cout=cout, ksize=k, dil=s["dil"], x=x, w=w, e=e, gate=gate, layout=layout,
                c_off=c_off, ld_out=c_off + cout + 3, where=where)


def _nchw(x, c):
    return x[:, :, :c["cin"]].reshape(c["BN"], c["H"], c["W"], c["cin"]).permute(0, 3, 1, 2)


def _conv(c, x, w, dtype):
    """F.conv2d of the rows x with the packed weight w -> [BN,hw,Cout]"""
    k, cin, cout = c["ksize"], c["cin"], c["cout"]
    wv = w[:, :cin, :cout].reshape(k, k, cin, cout).permute(3, 2, 0, 1).to(dtype)
    y = TF.conv2d(_nchw(x, c).to(dtype), wv, padding=c["dil"] if k == 3 else 0, dilation=c["dil"])
    return y.reshape(c["BN"], cout, c["hw"]).permute(0, 2, 1)


def _gated(c, x, dtype):
    x = x[:, :, :c["cin"]].to(dtype).clone()
    if c["gate"] is not None:
        gc = c["gate"].shape[1]
        x[:, :, :gc] = x[:, :, :gc] * c["gate"].to(dtype).unsqueeze(1)
    return x


@functools.lru_cache(maxsize=None)
def conv_reference(name):
    """-> ref (float64), A, r32 (torch's float32 conv2d and epilogue), all [BN,hw,Cout]; read-only"""
    c = conv_case(name)
    with torch.no_grad():
        ref = epilogue(_conv(c, _gated(c, c["x"], F64), c["w"], F64), c["e"], F64)
        A = epilogue(_conv(c, torch.nan_to_num(_gated(c, c["x"], F64).abs()), c["w"].abs(), F64), c["e"], F64, magnitude=True)
        r32 = epilogue(_conv(c, _gated(c, c["x"], F32), c["w"], F32), c["e"], F32)
    return dict(ref=ref, A=torch.nan_to_num(A), r32=r32)


def launch_conv(run, c, x=None, w=None, BN=None):
    """one launch into a guarded destination -> [BN,hw,Cout] on the host; the destination's other channels must still be NaN"""
    n, hw, cout, c_off, ld_out, e = c["BN"], c["hw"], c["cout"], c["c_off"], c["ld_out"], c["e"]
    cf = c["layout"] == "cf"
    full, dst = guarded(run, n, (ld_out, c["H"], c["W"]) if cf else (hw, ld_out))
    dv = lambda t: run.dev(t.contiguous()) if t is not None else None                 # noqa: E731
    rc = run.conv_small(dv(c["x"] if x is None else x), dv(c["w"] if w is None else w), cout, c["H"], c["W"], ksize=c["ksize"], dilation=c["dil"],
                        cin=c["cin"], bias=dv(e.get("bias")), img_bias=dv(e.get("img_bias")), gate=dv(c["gate"]), residual=dv(e.get("residual")),
                        bins=dv(e.get("bins")), bins_table=dv(e.get("bins_table")), cls=dv(e.get("cls")), cls_table=dv(e.get("cls_table")),
                        relu=bool(e.get("relu")), out=dst, channel_first=cf, c_off=c_off, **({} if BN is None else {"BN": BN}))
    require(rc == 0, f"{c['name']}: rc {rc}")
    got = taken(run, full, n)
    got = got.reshape(n, ld_out, hw).permute(0, 2, 1) if cf else got
    rest = torch.cat([got[:, :, :c_off].flatten(), got[:, :, c_off + cout:].flatten()])
    require(bool(torch.isnan(rest).all()), f"{c['name']}: {int((~torch.isnan(rest)).sum())} words written outside channels {c_off}..{c_off + cout - 1}")
    return got[:, :, c_off:c_off + cout]


def footprint(c):
    """the output elements that read the poisoned input pixel: the live taps' dilated footprint, every channel, that image"""
    n, p, _ = c["where"]
    h, w = divmod(p, c["W"])
    fp = torch.zeros(c["BN"], c["H"], c["W"], c["cout"], dtype=torch.bool)
    for tp in live_taps(c["H"], c["W"], c["ksize"], c["dil"]):
        dy, dx = tap_offset(tp, c["ksize"], c["dil"])
        if 0 <= h - dy < c["H"] and 0 <= w - dx < c["W"]:
            fp[n, h - dy, w - dx] = True
    return fp.reshape(c["BN"], c["hw"], c["cout"])


def expected_nan(c):
    """where a poisoned case's float64 reference has to be NaN"""
    what, n = c["spec"]["poison"], POISON_IMAGE
    m = torch.zeros(c["BN"], c["hw"], c["cout"], dtype=torch.bool)
    if what == "input":
        return footprint(c)
    if what == "gate":
        m[n] = True
    elif what == "residual":
        m[c["where"]] = True
    elif what == "img_bias":
        m[n, :, c["where"][1]] = True
    elif what == "bins_row":
        m[c["e"]["bins"].reshape(c["BN"], -1) == 3] = True
    else:
        k = c["e"]["cls"].reshape(c["BN"], -1)
        m[:, :, 4] = (k < 0) | (k >= N_CLS)
    return m


def check_conv(log, name, run):
    """one case of cs_conv_kernel against float64, with what its flags add"""
    c, r = conv_case(name), conv_reference(name)
    s, H, W, BN = c["spec"], c["H"], c["W"], c["BN"]
    taps = live_taps(H, W, c["ksize"], c["dil"], fault=getattr(run, "fault", None))
    if "taps" in s:
        require(taps == s["taps"], f"{name}: the tap rule gives {taps}, not {s['taps']}")
    tiles, last = conv_tiles(H, W)
    key = f"conv_small {'channel-first' if c['layout'] == 'cf' else 'channel-last'} | {name}"
    parts = [p for p in ALL_PARTS if p in s["parts"]]
    which = "all together" if len(parts) == len(ALL_PARTS) else parts[0] + " alone" if len(parts) == 1 else "some" if parts else "none"
    log.reached |= {f"conv tiles {min(tiles, 2)}", f"conv {'ragged' if last < CS_TM else 'whole'} last tile",
                    f"conv taps {TAP_SETS[live_taps(H, W, c['ksize'], c['dil'])]}", f"conv chunks {c['cin'] // CS_TK}",
                    f"conv cout {cout_class(c['cout'])}", f"conv layout {c['layout']}", "conv epilogue " + which}
    if len(taps) == 3:
        log.reached.add("conv taps six dead of nine")
    if c["gate"] is not None:
        log.reached.add("conv gate " + ("all channels" if c["gate"].shape[1] == c["cin"] else "some channels"))
    if s.get("poison"):
        nan = torch.isnan(r["ref"])
        assert torch.equal(nan, expected_nan(c)), f"{name}: float64's NaN set is not the elements that read the poisoned value"
        assert bool(nan.any())
        if s["poison"] in ("input", "gate", "residual", "img_bias"):
            assert not bool(nan[[n for n in range(BN) if n != POISON_IMAGE]].any()), f"{name}: another image is NaN in float64"
        if s["poison"] == "input":
            assert int(nan.sum()) == len(live_taps(H, W, c["ksize"], c["dil"])) * c["cout"], f"{name}: a live tap's footprint leaves the map"
    out = launch_conv(run, c)
    log.compare(key + " | out", out, r["ref"], r["A"], r["r32"], lolo=False)
    if "small_image" in s:
        n = s["small_image"]
        assert float(r["A"][n].max()) < 2.0 ** -9 * float(r["A"].max())
        log.compare(f"{key} | the image x 2^-12", out[n], r["ref"][n], r["A"][n], r["r32"][n], lolo=False)
    if s.get("zero"):                                     # the epilogue's constants in the kernel's order, bit for bit
        want = epilogue(torch.zeros(BN, c["hw"], c["cout"]), c["e"], F32)
        require(image_equal(out.contiguous(), want.contiguous()), f"{key}: an all-zero {s['zero']} does not give the epilogue's bits")
    if "pow2" in s:                                       # conv(2^k x) == 2^k conv(x), bit for bit (no epilogue term)
        base = launch_conv(run, c, x=c["x"] * 2.0 ** -s["pow2"])
        require(bits_equal((base * 2.0 ** s["pow2"]).contiguous(), out.contiguous()), f"{key}: conv(2^k x) != 2^k conv(x)")
    return out


def check_conv_bn0(run):
    """BN = 0 returns 0 with nothing written: the whole guarded buffer, the launch's own channels included, still NaN"""
    for name in ("7x11 k1 everything channel-first", "8x8 d1 96->96 gate 32 everything"):
        out = launch_conv(run, conv_case(name), BN=0)
        require(bool(torch.isnan(out).all()), f"{name}: BN = 0 wrote something")


# =============================================================================================== stage C: the vector kernels
# (C, BN, branches, what)
GATES_CASES = {"C1": (1, 1, 1, None), "C9": (9, 3, 2, None), "C256": (256, 3, 3, None), "C257": (257, 1, 2, None), "C1024": (1024, 3, 1, None),
               "C256 saturated": (256, 3, 2, "saturated"), "C257 poison": (257, 3, 3, "poison"), "C9 poison": (9, 3, 1, "poison")}
SATURATED = {3: 150.0, 8: -150.0}                        # be of these channels: the sigmoid is exactly 1 / exactly 0 in float32


def _split_block(p, C):
    sizes = (9 * C, C, C * C, C, C * C, C, C * C, C)
    w1, b1, w2, b2, wr, br, we, be = torch.split(p, sizes)
    return w1.view(9, C), b1, w2.view(C, C), b2, wr.view(C, C), br, we.view(C, C), be


@functools.lru_cache(maxsize=None)
def gates_case(name):
    C, BN, branches, what = GATES_CASES[name]
    g = torch.Generator().manual_seed(8000 + list(GATES_CASES).index(name))
    mlp = torch.randn(BN, 9, generator=g)                                         # (rows differ per image)
    blocks = []
    for _ in range(branches):
        parts = [torch.randn(9, C, generator=g) / 3.0, torch.randn(C, generator=g) * 0.3]
        for _ in range(3):
            parts += [torch.randn(C, C, generator=g) / math.sqrt(C), torch.randn(C, generator=g) * 0.3]
        if what == "saturated":
            for ch, v in SATURATED.items():
                parts[7][ch] = v
        blocks.append(torch.cat([p.reshape(-1) for p in parts]))
    params = torch.stack(blocks)
    assert params.shape[1] == gates_block(C)
    if what == "poison":
        mlp[POISON_IMAGE, 4] = NAN
    with torch.no_grad():
        ref, r32, A = [], [], []
        for b in range(branches):
            w1, b1, w2, b2, wr, br, we, be = _split_block(params[b], C)
            out = {}
            for dt in (F64, F32):
                x = mlp.to(dt)
                s1 = x @ w1.to(dt) + b1.to(dt)
                s2 = torch.relu(s1) @ w2.to(dt) + b2.to(dt)
                s3 = s2 @ wr.to(dt) + br.to(dt)                        # (Mlp.fc2 has no activation behind it)
                s4 = torch.relu(s3) @ we.to(dt) + be.to(dt)
                out[dt] = (s1, s2, s3, s4)
            a = mlp.double().abs()
            for s, w_, b_ in zip(out[F64], (w1, w2, wr, we), (b1, b2, br, be)):
                a = a @ w_.double().abs() + b_.double().abs() + s.abs()
            ref.append(torch.sigmoid(out[F64][3]))
            r32.append(torch.sigmoid(out[F32][3]))
            A.append(torch.nan_to_num(a) / 4)
    return dict(C=C, BN=BN, branches=branches, what=what, mlp=mlp, params=params, ref=torch.stack(ref), r32=torch.stack(r32), A=torch.stack(A))


def check_gates(log, name, run):
    c = gates_case(name)
    C, BN, branches = c["C"], c["BN"], c["branches"]
    log.reached |= {f"gates {'c += 256 loop' if C > 256 else 'one trip'}", f"gates branches {branches}", f"gates BN {BN}"}
    full, dst = guarded(run, branches, (BN, C))
    run.gates(run.dev(c["mlp"]), run.dev(c["params"]), dst, BN, C, branches)
    got = taken(run, full, branches)
    if c["what"] == "poison":
        nan = torch.isnan(c["ref"])
        assert bool(nan[:, POISON_IMAGE].all()) and int(nan.sum()) == branches * C, "float64: the poisoned image's gates, every branch, no others"
    log.compare(f"gates | {name} | gates", got, c["ref"], c["A"], c["r32"], R=2.0 ** -22 * torch.nan_to_num(c["ref"].abs()), lolo=False)
    if c["what"] == "saturated":
        for ch, v in SATURATED.items():
            want = c["ref"][:, :, ch].float()
            assert bool((want == (1.0 if v > 0 else 0.0)).all()), "float64 rounded to float32 is not saturated"
            require(bits_equal(got[:, :, ch].contiguous(), want.contiguous()), f"gates {name}: channel {ch} is not exactly {1 if v > 0 else 0}")


# (C, hw, ld, Cout, BN, poison): G = 1024, 10, 4, 3, 1; hw 1 and 3 leave segments empty; 96 and 300 leave threads idle
POOL_CASES = {"C1 hw1": (1, 1, 2, 1, 1, False), "C1 hw704": (1, 704, 3, 256, 3, False), "C96 hw3": (96, 3, 100, 256, 3, False),
              "C256 hw704": (256, 704, 260, 256, 3, False), "C300 hw15": (300, 15, 304, 1100, 1, False), "C1024 hw704": (1024, 704, 1027, 1, 1, False),
              "C1024 hw15": (1024, 15, 1028, 1100, 3, False), "C256 hw704 poison": (256, 704, 260, 256, 3, True), "C96 hw15 poison": (96, 15, 99, 1100, 3, True)}


@functools.lru_cache(maxsize=None)
def pool_case(name):
    C, hw, ld, Cout, BN, poison = POOL_CASES[name]
    g = torch.Generator().manual_seed(9000 + list(POOL_CASES).index(name))
    x = torch.full((BN, hw, ld), NAN)                                            # (the columns behind C unread)
    x[:, :, :C] = torch.randn(BN, hw, C, generator=g)
    wp, bp = torch.randn(C, C, generator=g) / math.sqrt(C), torch.randn(C, generator=g) * 0.3
    wb = torch.randn(C, Cout, generator=g) / math.sqrt(C)
    if poison:
        x[POISON_IMAGE, hw - 2, C // 2] = NAN
    with torch.no_grad():
        out = {}
        for dt in (F64, F32):
            m = x[:, :, :C].to(dt).mean(1)
            out[dt] = torch.relu(m @ wp.to(dt) + bp.to(dt)) @ wb.to(dt)
        A = (torch.nan_to_num(x[:, :, :C].double().abs()).mean(1) @ wp.double().abs() + bp.double().abs()) @ wb.double().abs()
    return dict(C=C, hw=hw, ld=ld, Cout=Cout, BN=BN, poison=poison, x=x, wp=wp, bp=bp, wb=wb, ref=out[F64], r32=out[F32], A=A)


def check_pool(log, name, run):
    c = pool_case(name)
    C, hw, BN = c["C"], c["hw"], c["BN"]
    G, segs = pool_segments(hw, C)
    log.reached |= {f"pool G {G}", f"pool Cout {c['Cout']}"}
    if any(a == b for a, b in segs):
        log.reached.add("pool empty segments")
    if G * C < DN_THREADS:
        log.reached.add("pool idle threads")
    full, dst = guarded(run, BN, (c["Cout"],))
    run.pool_bias(run.dev(c["x"]), run.dev(c["wp"]), run.dev(c["bp"]), run.dev(c["wb"]), dst, BN, hw, c["ld"], C, c["Cout"])
    got = taken(run, full, BN)
    if c["poison"]:
        nan = torch.isnan(c["ref"])
        assert bool(nan[POISON_IMAGE].all()) and int(nan.sum()) == c["Cout"], "float64: the poisoned image's whole bias, no other's"
    log.compare(f"pool_bias | {name} | img_bias", got, c["ref"], c["A"], c["r32"], lolo=False)


# =============================================================================================== the restatement and its faults
FAULTS = ("dy_dx_exchanged", "dead_tap_le", "dead_tap_not_zeroed", "gate_past_channels", "other_image_gate", "bins_row_for_n_bins",
          "cls_without_plus_1", "cls_out_of_range_adds_nothing", "residual_ld_out", "relu_before_residual", "relu_drops_nan", "c_off_ignored_cf",
          "pack_padding_unwritten", "pool_mean_by_segment_length", "pool_last_pixel_dropped", "branch1_reads_branch0", "gates_relu_drops_nan",
          "pool_relu_drops_nan")
# the case each control is run on, as (check, case).  dead_tap_le: a tap at |offset| == extent reads padding alone and adds an exact
# zero, so on the device the variant costs time and changes no bit; it is caught in the rule restated (6 x 7 at dilation 6), the rule
# the reach assertions rest on.
FAULT_CASES = {"dy_dx_exchanged": ("conv", "20x23 d6"), "dead_tap_le": ("conv", "6x7 d6"), "dead_tap_not_zeroed": ("conv", "7x11 d1 no epilogue"),
               "gate_past_channels": ("conv", "7x11 d1 gate 32 of 96"), "other_image_gate": ("conv", "7x11 k1 gate all"),
               "bins_row_for_n_bins": ("conv", "7x11 k1 bins alone"), "cls_without_plus_1": ("conv", "7x11 k1 cls alone"),
               "cls_out_of_range_adds_nothing": ("conv", "7x11 k1 cls alone"), "residual_ld_out": ("conv", "7x11 k1 residual alone"),
               "relu_before_residual": ("conv", "8x8 d1 256->256 residual"), "relu_drops_nan": ("conv", "poison input 20x23 d6 relu"),
               "c_off_ignored_cf": ("conv", "7x11 k1 everything channel-first"), "pack_padding_unwritten": ("pack", "C31 hw31"),
               "pool_mean_by_segment_length": ("pool", "C256 hw704"), "pool_last_pixel_dropped": ("pool", "C96 hw3"),
               "branch1_reads_branch0": ("gates", "C9"), "gates_relu_drops_nan": ("gates", "C257 poison"), "pool_relu_drops_nan": ("pool", "C256 hw704 poison")}
# "the partial sums of a K step chained on instead of restarted" is not among them: it changes the rounding alone (measured in
# tests/test_depth_net_fwd_f64_cpu.py::test_chained_k_steps_stay_inside_the_bound) and can fail no check.


class Restated:
    """the runner of the CPU module; ``fault``: one of FAULTS (or "k_step_chained"), the deliberately wrong variant of a control"""

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS or fault == "k_step_chained"
        self.fault = fault

    def dev(self, t):
        return t

    def host(self, t):
        return t

    def pack_rows(self, src, dst, c_off=0, c_pad=0, BN=None):
        n, C, hw = src.shape[:3]
        if BN == 0:
            return 0
        dst[:, :, c_off:c_off + C] = src.reshape(n, C, hw).permute(0, 2, 1)
        if self.fault != "pack_padding_unwritten":
            dst[:, :, c_off + C:c_off + C + c_pad] = 0.0
        return 0

    def conv_small(self, x, w, cout, H, W, ksize=1, dilation=1, cin=None, bias=None, img_bias=None, gate=None, residual=None, bins=None,
                   bins_table=None, cls=None, cls_table=None, relu=False, out=None, channel_first=False, c_off=0, BN=None):
        f = self.fault
        if BN == 0:
            return 0
        n, hw, _ = x.shape
        cin = w.shape[1] if cin is None else cin
        chunks = cin // CS_TK
        xg = x[:, :, :cin].clone()
        if gate is not None:                              # multiplied in while the operand is staged: one float32 rounding
            gc = gate.shape[1]
            gv = gate[[(i + 1) % n for i in range(n)]] if f == "other_image_gate" else gate
            if f == "gate_past_channels":
                xg = xg * gv[:, torch.arange(cin) % gc].unsqueeze(1)
            else:
                xg[:, :, :gc] = xg[:, :, :gc] * gv.unsqueeze(1)
        xg = xg.reshape(n, H, W, cin)
        acc = torch.zeros(n, hw, cout)
        for tp in live_taps(H, W, ksize, dilation, f):
            dy, dx = tap_offset(tp, ksize, dilation)
            if f == "dy_dx_exchanged":
                dy, dx = dx, dy
            a = shifted(xg, dy, dx, zero=f != "dead_tap_not_zeroed").reshape(n, hw, chunks, CS_TK).permute(2, 0, 1, 3)
            b = w[tp, :cin, :cout].reshape(chunks, 1, CS_TK, cout)
            if f == "k_step_chained":
                for k in range(chunks):
                    acc = fma_chain(a[k], b[k], acc)
                continue
            part = fma_chain(a, b, torch.zeros(chunks, n, hw, cout))
            for k in range(chunks):
                acc = acc + part[k]
        ld_out = out.shape[1] if channel_first else out.shape[2]
        e = dict(bias=bias, img_bias=img_bias, bins=bins, bins_table=bins_table, cls=cls, cls_table=cls_table, residual=residual, relu=relu)
        v = epilogue(acc, e, F32, fault=f, ld_out=ld_out)
        if channel_first:
            o = 0 if f == "c_off_ignored_cf" else c_off
            out[:, o:o + cout] = v.permute(0, 2, 1).reshape(n, cout, H, W)
        else:
            out[:, :, c_off:c_off + cout] = v
        return 0

    def gates(self, mlp, params, out, BN, C, branches):
        f = self.fault
        for b in range(branches):
            w1, b1, w2, b2, wr, br, we, be = _split_block(params[0 if f == "branch1_reads_branch0" and b == 1 else b], C)
            rl = (lambda t: relu(t, "relu_drops_nan")) if f == "gates_relu_drops_nan" else relu
            u = rl(fma_chain(mlp, w1, b1.expand(BN, C)))
            v = fma_chain(u, w2, b2.expand(BN, C))
            u = rl(fma_chain(v, wr, br.expand(BN, C)))
            s = fma_chain(u, we, be.expand(BN, C))
            out[b] = 1.0 / (1.0 + torch.exp(-s))

    def pool_bias(self, x, wp, bp, wb, out, BN, hw, ld, C, Cout):
        f = self.fault
        G, segs = pool_segments(hw, C)
        total = None
        for q0, q1 in segs:
            s = torch.zeros(BN, C)
            for q in range(q0, q1 - (1 if f == "pool_last_pixel_dropped" else 0)):
                s = s + x[:, q, :C]
            total = s if total is None else total + s
        n = float(segs[0][1] - segs[0][0] or hw) if f == "pool_mean_by_segment_length" else float(hw)
        m = total / torch.tensor(n, dtype=F32)
        y = relu(fma_chain(m, wp, bp.expand(BN, C)), "relu_drops_nan" if f == "pool_relu_drops_nan" else None)
        out.copy_(fma_chain(y, wb, torch.zeros(BN, Cout)))


def check_pack_case(log, name, run):
    check_pack(run, name)


CHECKS = {"conv": check_conv, "pack": check_pack_case, "gates": check_gates, "pool": check_pool}

# what a whole session has to reach (asserted by both modules once every case has run)
REACH = {"conv tiles 1", "conv tiles 2", "conv whole last tile", "conv ragged last tile", "conv taps six dead of nine", "conv layout cl", "conv layout cf",
         "conv gate all channels", "conv gate some channels", "conv epilogue none", "conv epilogue all together", "pool empty segments", "pool idle threads",
         "gates one trip", "gates c += 256 loop"} \
    | {f"conv taps {v}" for v in TAP_SETS.values()} | {f"conv chunks {k}" for k in (1, 3, 8, 32)} \
    | {f"conv cout {cout_class(k)}" for k in (1, 24, 33, 64, 96, 256)} | {f"conv epilogue {p} alone" for p in ALL_PARTS} \
    | {f"pool G {g}" for g in (1024, 10, 4, 3, 1)} | {f"pool Cout {k}" for k in (1, 256, 1100)} | {f"gates branches {k}" for k in (1, 2, 3)} \
    | {f"gates BN {k}" for k in (1, 3)}
