#!/usr/bin/env python3
"""Pin of the image-side convolution family as a given build of libracformer_hip.so computes it (MI355X only), on seeded
inputs.  Writes conv_family_pin.json: the SHA-256 of every input array and of every output -- a bit-for-bit pin of a few
KiB -- over the smallest cases that reach every instance of the kernels that share code:

  * rac_resnet_conv_fwd / rac_resnet_conv_dgrad (rn_conv_kernel, both rules): 64 channels per workgroup on 64 -> 64 3x3 s1 at
    7x11 x 2 and 128 -> 128 3x3 s2 at 7x11 x 2 and 8x8 x 1 (a ragged tile, border taps, odd and even stride-2 sizes), each with every
    epilogue operand and with none; 256 and 128 channels on 64 -> 256 1x1 at 64x64 with 4 and 3 images (the data gradient: of
    256 -> 64), the two sides of the 256-workgroup switch;
  * rac_resnet_conv_wgrad, dW and db: the 128 x 128 tile (192 -> 128 1x1, a ragged second ci tile), the 64 x 64 tile (160 -> 64 3x3 s2),
    and 64 -> 64 3x3 s1 at 16x44 x 3 with k_splits = 1, the default and 5 (which does not divide the 66 units);
  * rac_fpn_lateral_wgrad, dW and db: 16-byte and 4-byte loads on the 64- and the 128-channel ci tile at the default k_splits, the
    common 256-channel level also at 1;
  * rac_fpn_lateral_fwd / rac_fpn_lateral_dgrad, rac_conv3x3_wgrad and rac_linear_wgrad in both orientations, which share the
    operand types and the transposed LDS read.

tests/test_conv_family_pin_gpu.py checks that the current build returns them bit for bit (the input digests tell a change of
the seeded inputs apart from one of the kernels).  The library is loaded on its own and takes the place of the package's:
    python tests/golden/gen_conv_family_pin.py --lib path/to/libracformer_hip.so [--out tests/golden/conv_family_pin.json]
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from racformer_amd import _lib  # noqa: E402

DEV = "cuda:0"
# (name, Cin, Cout, ksize, stride, H, W, images): the convolution; its data gradient is that of the same convolution
NARROW = [("c64_k3s1_7x11", 64, 64, 3, 1, 7, 11, 2), ("c128_k3s2_7x11", 128, 128, 3, 2, 7, 11, 2), ("c128_k3s2_8x8", 128, 128, 3, 2, 8, 8, 1)]
WIDE_FWD = [("c256_k1_64x64x4", 64, 256, 1, 1, 64, 64, 4, 256), ("c256_k1_64x64x3", 64, 256, 1, 1, 64, 64, 3, 128)]      # .., tile width
WIDE_DGRAD = [("c256_k1_64x64x4", 256, 64, 1, 1, 64, 64, 4, 256), ("c256_k1_64x64x3", 256, 64, 1, 1, 64, 64, 3, 128)]
# (name, Cin, Cout, ksize, stride, H, W, images, k_splits (None: the default))
RN_WGRAD = [("ragged128", 192, 128, 1, 1, 7, 11, 2, None), ("ragged64", 160, 64, 3, 2, 7, 11, 2, None),
            ("c64_16x44_k1", 64, 64, 3, 1, 16, 44, 3, 1), ("c64_16x44_default", 64, 64, 3, 1, 16, 44, 3, None),
            ("c64_16x44_k5", 64, 64, 3, 1, 16, 44, 3, 5)]
# (name, images, Cin, H, W, k_splits)
FPN_WGRAD = [("c32", 3, 32, 8, 22, None), ("odd", 2, 96, 7, 11, None), ("c256", 3, 256, 8, 22, None), ("c256_k1", 3, 256, 8, 22, 1),
             ("c160_odd", 2, 160, 7, 11, None)]
FPN_LATERAL = [("c32", 3, 32, 8, 22), ("odd", 2, 96, 7, 11)]
CONV3X3 = (2, 8, 12, 32)                                 # N, H, W, hidden channels: case C of test_temporal_fusion_grad_gpu.py
LINEAR = [(17, 128), (130, 384)]                         # rows M, wide side


def conv_out(h, k, s):
    return (h + 2 * (k // 2) - k) // s + 1


def inputs():
    rng = np.random.default_rng(2027)
    nrm = lambda *s: rng.standard_normal(s, dtype=np.float32)      # noqa: E731
    d = {}
    for name, ci, co, k, s, h, w, n, *_ in NARROW + WIDE_FWD:
        ho, wo = conv_out(h, k, s), conv_out(w, k, s)
        d[f"rn_{name}_x"] = nrm(n, ci, h, w)
        d[f"rn_{name}_w"] = nrm(co, ci, k, k) / np.float32(np.sqrt(ci * k * k))
        d[f"rn_{name}_b"] = nrm(co)
        d[f"rn_{name}_res"] = nrm(n, co, ho, wo)
    for name, ci, co, k, s, h, w, n, *_ in NARROW + WIDE_DGRAD:
        ho, wo = conv_out(h, k, s), conv_out(w, k, s)
        d[f"dg_{name}_g"] = nrm(n, co, ho, wo)
        d[f"dg_{name}_w"] = nrm(co, ci, k, k) / np.float32(np.sqrt(ci * k * k))
        d[f"dg_{name}_add"] = nrm(n, ci, h, w)
        d[f"dg_{name}_mask"] = np.maximum(nrm(n, ci, h, w), np.float32(0))
    for name, ci, co, k, s, h, w, n, _ in RN_WGRAD:
        if f"wg_{ci}_{co}_x" not in d:
            d[f"wg_{ci}_{co}_x"] = nrm(n, ci, h, w)
            d[f"wg_{ci}_{co}_g"] = nrm(n, co, conv_out(h, k, s), conv_out(w, k, s))
    for name, n, ci, h, w, _ in FPN_WGRAD:
        if f"fpn_{n}_{ci}_x" not in d:
            d[f"fpn_{n}_{ci}_x"] = nrm(n, ci, h, w)
            d[f"fpn_{n}_{ci}_g"] = nrm(n, 256, h, w)
            d[f"fpn_{n}_{ci}_w"] = nrm(256, ci, 1, 1) / np.float32(np.sqrt(ci))
            d[f"fpn_{n}_{ci}_b"] = nrm(256)
    n, h, w, hd = CONV3X3
    d["tf_x"], d["tf_hid"], d["tf_gy"] = nrm(n, 256, h, w), nrm(n, hd, h, w) * np.float32(0.5), nrm(n, h, w, 256)
    d["tf_w"], d["tf_b"] = nrm(256, 256 + hd, 3, 3) * np.float32(0.03), nrm(256) * np.float32(0.1)
    for m, wd in LINEAR:
        d[f"lin_{m}_{wd}_narrow"], d[f"lin_{m}_{wd}_wide"] = nrm(m, 256), nrm(m, wd)
    return d


def use_library(path):
    """the build at ``path`` in the place of the package's own: every wrapper of racformer_amd then calls it"""
    handle = ctypes.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(handle, name)
        fn.restype, fn.argtypes = res, args
    _lib._lib = handle


def outputs(d):
    """every pinned array of the library in use (``use_library``, or the package's own), by name"""
    from racformer_amd import fused, necks, resnet
    from racformer_amd import transformer as T
    t = lambda k: torch.from_numpy(d[k]).to(DEV)      # noqa: E731
    r = {}
    for name, ci, co, k, s, h, w, n, *width in NARROW + WIDE_FWD:
        assert not width or resnet.conv_tile_channels(co, n, conv_out(h, k, s), conv_out(w, k, s))[0] == width[0]
        x, packed = t(f"rn_{name}_x"), resnet.pack_conv_weight(t(f"rn_{name}_w"))
        r[f"rn_fwd_{name}_full"] = resnet.conv_fwd(x, packed, t(f"rn_{name}_b"), k, s, residual=t(f"rn_{name}_res"), relu=True)
        if not width:
            r[f"rn_fwd_{name}_plain"] = resnet.conv_fwd(x, packed, None, k, s, relu=False)
    for name, ci, co, k, s, h, w, n, *width in NARROW + WIDE_DGRAD:
        assert not width or resnet.conv_tile_channels(ci, n, h, w)[0] == width[0]
        g, packed = t(f"dg_{name}_g"), resnet.pack_conv_weight_t(t(f"dg_{name}_w"))
        r[f"rn_dgrad_{name}_full"] = resnet.conv_dgrad(g, packed, k, s, (h, w), add=t(f"dg_{name}_add"), mask=t(f"dg_{name}_mask"))
        if not width:
            r[f"rn_dgrad_{name}_plain"] = resnet.conv_dgrad(g, packed, k, s, (h, w))
    for name, ci, co, k, s, h, w, n, ks in RN_WGRAD:
        r[f"rn_wgrad_{name}_dw"], r[f"rn_wgrad_{name}_db"] = resnet.conv_wgrad(t(f"wg_{ci}_{co}_g"), t(f"wg_{ci}_{co}_x"), k, s, k_splits=ks)
    for name, n, ci, h, w, ks in FPN_WGRAD:
        r[f"fpn_wgrad_{name}_dw"], r[f"fpn_wgrad_{name}_db"] = necks.fpn_lateral_wgrad(t(f"fpn_{n}_{ci}_g"), t(f"fpn_{n}_{ci}_x"), k_splits=ks)
    for name, n, ci, h, w in FPN_LATERAL:
        wt = t(f"fpn_{n}_{ci}_w")
        r[f"fpn_fwd_{name}"] = necks.fpn_lateral(t(f"fpn_{n}_{ci}_x"), necks.pack_lateral_weight(wt), t(f"fpn_{n}_{ci}_b"))
        r[f"fpn_dgrad_{name}"] = necks.fpn_lateral_dgrad(t(f"fpn_{n}_{ci}_g"), necks.pack_lateral_weight_t(wt), ci)
    ts = [t(k).requires_grad_(k == "tf_w") for k in ("tf_x", "tf_hid", "tf_w", "tf_b")]
    ws, alpha = fused.pack_conv3x3_weight(ts[2])
    T._TemporalFusionCore.apply(*ts, dict(ws=ws, alpha=alpha)).backward(t("tf_gy"))
    r["conv3x3_wgrad_C"] = ts[2].grad
    for m, wd in LINEAR:
        narrow, wide = t(f"lin_{m}_{wd}_narrow"), t(f"lin_{m}_{wd}_wide")
        an, aw = fused.absmax_device(narrow), fused.absmax_device(wide)
        img = fused.linear_pack_act(narrow, an)
        r[f"linear_wgrad_{m}_{wd}_narrow_major"] = fused.linear_wgrad(img, an, wide, aw, False)
        r[f"linear_wgrad_{m}_{wd}_wide_major"], r[f"linear_wgrad_{m}_{wd}_colsum"] = fused.linear_wgrad(img, an, wide, aw, True, colsum=True)
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in r.items()}


def digest(a):
    """SHA-256 of an array's dtype, shape and bytes"""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "conv_family_pin.json"))
    args = ap.parse_args()
    use_library(args.lib)
    d = inputs()
    res = outputs(d)
    for k, v in res.items():
        assert np.isfinite(v).all(), k   # every element written
    pin = {"inputs": {k: digest(v) for k, v in sorted(d.items())}, "outputs": {k: digest(v) for k, v in sorted(res.items())}}
    with open(args.out, "w") as f:
        json.dump(pin, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}: {len(res)} outputs, {os.path.getsize(args.out) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
