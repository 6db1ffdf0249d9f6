#!/usr/bin/env python3
"""Pin of the gather forwards (and MSDA's single-writer gradients) as a given build of libracformer_hip.so computes them
(MI355X only), on seeded inputs with finite locations only, out-of-range ones included.  Writes gather_fwd_pin.json: the
SHA-256 of every input array and of every output -- a bit-for-bit pin that stays a few KiB where the arrays themselves
would take more than a MiB -- of every forward kernel instance:

  * rac_msmv_fwd: msmv_fwd_c64_kernel<FT, L, OUT_CL> for f32 / bf16, L = 2, 4, 5, both output layouts, and
    msmv_fwd_generic_kernel (C = 8, and C = 64 at L = 3) for f32 / bf16;
  * rac_msmv_v2_fwd: the C = 64 and generic kernels for f32 / bf16, channel-last, and channel-first f32;
  * rac_msda_fwd: msda_fwd_d64_kernel and msda_fwd_generic_kernel for f32 / bf16;
  * rac_msda_bwd: grad_loc / grad_attn of msda_bwd_d64_kernel and msda_bwd_generic_kernel.

tests/test_gather_pin_gpu.py checks that the current build returns them bit for bit (the input digests tell a change of
the seeded inputs apart from one of the kernels).  The library is loaded on its own (not through racformer_amd._lib):
    python tests/golden/gen_gather_fwd_pin.py --lib path/to/libracformer_hip.so [--out tests/golden/gather_fwd_pin.json]
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
from racformer_amd._lib import SIGNATURES  # noqa: E402

RAC_F32, RAC_BF16 = 0, 1
OUT_SQCP, OUT_BQGTPC = 0, 1
FEAT_CL, FEAT_CF = 0, 1

# msmv: pyramid, sizes, and the [B,Q,G,T*P,C] regroup (S = B*T*G, B = 1)
HWS = [(5, 9), (3, 5), (2, 3), (1, 4), (4, 1)]
S, N, Q, P = 4, 2, 9, 5             # Q = 9: two row blocks of the C = 64 kernel per slot, the second one partial
T_, G_ = 2, 2
# finite edges: map corners, just outside, far outside (the guard keeps them away from the float -> int conversion)
EDGES = [(0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (-0.1, 0.5, 0.0), (0.5, 1.2, 1.0), (5 / 8, 1 / 4, 0.0), (-3.0, 0.5, 1.0),
         (1e30, 0.5, 0.0), (0.5, -1e30, 1.0), (1.0 + 1e-7, -1e-7, 0.0)]
# msda: value [bs, keys, heads, dim], levels stacked along keys
MSDA_HWS = [(6, 7), (3, 4), (2, 2)]
BS, HEADS, MQ, MP = 2, 4, 10, 5
MSDA_EDGES = [(0.0, 0.0), (1.0, 1.0), (-0.2, 0.5), (0.5, 1.3), (1e30, 0.5), (0.5, -1e30), (1 / 14, 1 / 12)]

# (name, C, L, dtype, out_layout)
MSMV_CASES = [(f"v1_c64_l{L}_{dt}_{lay}", 64, L, dt, lay) for L in (2, 4, 5) for dt in ("f32", "bf16")
              for lay in ("sqcp", "bqgtpc")]
MSMV_CASES += [(f"v1_generic_c8_{dt}_{lay}", 8, 4, dt, lay) for dt in ("f32", "bf16") for lay in ("sqcp", "bqgtpc")]
MSMV_CASES += [(f"v1_generic_c64_l3_{dt}", 64, 3, dt, "sqcp") for dt in ("f32", "bf16")]
# (name, C, L, dtype, out_layout, channels_first)
V2_CASES = [(f"v2_c64_{dt}_{lay}", 64, 4, dt, lay, False) for dt in ("f32", "bf16") for lay in ("sqcp", "bqgtpc")]
V2_CASES += [(f"v2_generic_c8_{dt}_{lay}", 8, 4, dt, lay, False) for dt in ("f32", "bf16") for lay in ("sqcp", "bqgtpc")]
V2_CASES += [(f"v2_cf_c{C}_{lay}", C, 4, "f32", lay, True) for C in (64, 8) for lay in ("sqcp", "bqgtpc")]
# (name, dim, dtype); the backward cases are the f32 ones
MSDA_CASES = [(f"msda_d{D}_{dt}", D, dt) for D in (64, 8) for dt in ("f32", "bf16")]


def inputs():
    rng = np.random.default_rng(2026)
    d = {}
    for C in (64, 8):
        for i, (h, w) in enumerate(HWS):
            d[f"c{C}_feat{i}"] = rng.standard_normal((S, N, h, w, C), dtype=np.float32)
    loc = rng.random((S, Q, P, 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    loc[..., 2] = rng.integers(0, N, size=(S, Q, P)).astype(np.float32) / np.float32(N - 1)
    loc.reshape(-1, 3)[:len(EDGES)] = np.array(EDGES, dtype=np.float32)
    d["loc"] = loc
    d["w"] = rng.standard_normal((S, Q, P, len(HWS)), dtype=np.float32)
    keys = sum(h * w for h, w in MSDA_HWS)
    for D in (64, 8):
        d[f"msda_d{D}_value"] = rng.standard_normal((BS, keys, HEADS, D), dtype=np.float32)
        d[f"msda_d{D}_gout"] = rng.standard_normal((BS, MQ, HEADS * D), dtype=np.float32)
    mloc = rng.random((BS, MQ, HEADS, len(MSDA_HWS), MP, 2), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    mloc.reshape(-1, 2)[:len(MSDA_EDGES)] = np.array(MSDA_EDGES, dtype=np.float32)
    d["msda_loc"] = mloc
    d["msda_attn"] = rng.random((BS, MQ, HEADS, len(MSDA_HWS), MP), dtype=np.float32)
    return d


def _bind(lib, name):
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = SIGNATURES[name]
    return fn


def _dev(a, dt="f32", dev="cuda:0"):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return t.to(torch.bfloat16) if dt == "bf16" else t


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _hw(L):
    return (ctypes.c_int32 * (2 * L))(*[x for h_w in HWS[:L] for x in h_w])


def _out(lay, C):
    shape = (S, Q, C, P) if lay == "sqcp" else (S // (T_ * G_), Q, G_, T_ * P, C)
    return torch.full(shape, float("nan"), device="cuda:0")


def run_msmv(lib, d, C, L, dt, lay):
    """output of rac_msmv_fwd of `lib` on one case"""
    feats = [_dev(d[f"c{C}_feat{l}"], dt) for l in range(L)]
    loc, w, out = _dev(d["loc"]), _dev(d["w"][..., :L]), _out(lay, C)
    ptrs = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats])
    rc = _bind(lib, "rac_msmv_fwd")(ptrs, _hw(L), L, _p(loc), _p(w), _p(out), S, N, Q, P, C,
                                    RAC_BF16 if dt == "bf16" else RAC_F32, OUT_BQGTPC if lay == "bqgtpc" else OUT_SQCP,
                                    T_, G_, None)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_v2(lib, d, C, L, dt, lay, cf):
    """output of rac_msmv_v2_fwd of `lib` on one case"""
    feats = [_dev(d[f"c{C}_feat{l}"], dt) for l in range(L)]
    if cf:
        feats = [f.permute(0, 4, 1, 2, 3).contiguous() for f in feats]
    loc, w, out = _dev(d["loc"]), _dev(d["w"][..., :L]), _out(lay, C)
    ptrs = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats])
    rc = _bind(lib, "rac_msmv_v2_fwd")(ptrs, _hw(L), L, _p(loc), _p(w), _p(out), S, N, Q, P, C,
                                       RAC_BF16 if dt == "bf16" else RAC_F32, FEAT_CF if cf else FEAT_CL,
                                       OUT_BQGTPC if lay == "bqgtpc" else OUT_SQCP, T_, G_, None)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _msda_tables():
    shapes = (ctypes.c_int64 * (2 * len(MSDA_HWS)))(*[x for h_w in MSDA_HWS for x in h_w])
    starts = np.cumsum([0] + [h * w for h, w in MSDA_HWS])[:-1]
    return shapes, (ctypes.c_int64 * len(MSDA_HWS))(*[int(s) for s in starts]), int(sum(h * w for h, w in MSDA_HWS))


def run_msda_fwd(lib, d, D, dt):
    value, loc, attn = _dev(d[f"msda_d{D}_value"], dt), _dev(d["msda_loc"]), _dev(d["msda_attn"])
    out = torch.full((BS, MQ, HEADS * D), float("nan"), device="cuda:0")
    shapes, starts, keys = _msda_tables()
    rc = _bind(lib, "rac_msda_fwd")(_p(value), shapes, starts, _p(loc), _p(attn), _p(out), BS, keys, HEADS, D, MQ,
                                    len(MSDA_HWS), MP, RAC_BF16 if dt == "bf16" else RAC_F32, None)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy()


def run_msda_bwd(lib, d, D):
    """(grad_loc, grad_attn) of rac_msda_bwd of `lib`: the single-writer gradients"""
    value, loc, attn, gout = (_dev(d[k]) for k in (f"msda_d{D}_value", "msda_loc", "msda_attn", f"msda_d{D}_gout"))
    gvalue = torch.zeros_like(value)
    gloc, gattn = torch.full_like(loc, float("nan")), torch.full_like(attn, float("nan"))
    shapes, starts, keys = _msda_tables()
    rc = _bind(lib, "rac_msda_bwd")(_p(gout), _p(value), shapes, starts, _p(loc), _p(attn), _p(gvalue), _p(gloc),
                                    _p(gattn), BS, keys, HEADS, D, MQ, len(MSDA_HWS), MP, None)
    assert rc == 0
    torch.cuda.synchronize()
    return gloc.cpu().numpy(), gattn.cpu().numpy()


def outputs(lib, d):
    """every pinned array of `lib`, by name"""
    r = {}
    for name, C, L, dt, lay in MSMV_CASES:
        r[name] = run_msmv(lib, d, C, L, dt, lay)
    for name, C, L, dt, lay, cf in V2_CASES:
        r[name] = run_v2(lib, d, C, L, dt, lay, cf)
    for name, D, dt in MSDA_CASES:
        r[name] = run_msda_fwd(lib, d, D, dt)
        if dt == "f32":
            r[name + "_gloc"], r[name + "_gattn"] = run_msda_bwd(lib, d, D)
    return r


def digest(a):
    """SHA-256 of an array's dtype, shape and bytes"""
    a = np.ascontiguousarray(a)
    return hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "gather_fwd_pin.json"))
    args = ap.parse_args()
    lib = ctypes.CDLL(os.path.abspath(args.lib))
    d = inputs()
    res = outputs(lib, d)
    for k, v in res.items():
        assert np.isfinite(v).all(), k   # every element written, no non-finite location
    pin = {"inputs": {k: digest(v) for k, v in sorted(d.items())}, "outputs": {k: digest(v) for k, v in sorted(res.items())}}
    with open(args.out, "w") as f:
        json.dump(pin, f, indent=1)
        f.write("\n")
    print(f"wrote {args.out}: {len(res)} outputs, {os.path.getsize(args.out) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
