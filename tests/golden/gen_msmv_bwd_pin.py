#!/usr/bin/env python3
"""Pin of the single-writer gradients of rac_msmv_bwd / rac_msmv_v2_bwd as a given build of libracformer_hip.so computes
them (MI355X only).  Writes msmv_bwd_pin.npz: seeded inputs and grad_loc / grad_w of every backward kernel instance --
msmv_bwd_c64_kernel<L> for L = 2, 4, 5, msmv_bwd_generic_kernel, msmv_v2_bwd_c64_kernel and msmv_v2_bwd_generic_kernel
(channel-last and channel-first) -- with grad_out in [S,Q,C,P].  tests/test_sampling4d_grad_gpu.py checks that the current
build returns them bit for bit, through the old entry points and through the _ex ones in both gradient layouts.

The library is loaded on its own (not through racformer_amd._lib), so the pin can be made with a build that predates the
_ex entry points:
    python tests/golden/gen_msmv_bwd_pin.py --lib path/to/libracformer_hip.so [--out tests/golden/msmv_bwd_pin.npz]
"""
import argparse
import ctypes
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
HWS = [(5, 9), (3, 5), (2, 3), (1, 4), (4, 1)]
S, N, Q, P = 4, 2, 16, 6
T_, G_ = 2, 2                      # the BQGTPC regroup the test reads the same gradients in (S = B*T*G, B = 1)
EDGES = [(5 / 8, 1 / 4, 0.0), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (-0.1, 0.5, 0.0), (0.5, 1.2, 1.0), (float("nan"), 0.5, 0.0),
         (0.5, float("inf"), 1.0), (-float("inf"), 0.5, 0.0)]


def inputs():
    rng = np.random.default_rng(77)
    d = {}
    for C in (64, 8):
        for i, (h, w) in enumerate(HWS):
            d[f"c{C}_feat{i}"] = rng.standard_normal((S, N, h, w, C), dtype=np.float32)
        d[f"c{C}_gout"] = rng.standard_normal((S, Q, C, P), dtype=np.float32)
    loc = rng.random((S, Q, P, 3), dtype=np.float32) * np.float32(1.2) - np.float32(0.1)
    loc[..., 2] = rng.integers(0, N, size=(S, Q, P)).astype(np.float32) / np.float32(N - 1)
    loc.reshape(-1, 3)[:len(EDGES)] = np.array(EDGES, dtype=np.float32)
    d["loc"] = loc
    d["w"] = rng.random((S, Q, P, len(HWS)), dtype=np.float32) + np.float32(0.05)
    return d


# (name, C, L, v2, channels_first)
CASES = [("v1_c64_l2", 64, 2, False, False), ("v1_c64_l4", 64, 4, False, False), ("v1_c64_l5", 64, 5, False, False),
         ("v1_generic_l4", 8, 4, False, False), ("v2_c64_l4", 64, 4, True, False), ("v2_generic_l4", 8, 4, True, False),
         ("v2_cf_l4", 64, 4, True, True)]


def run_old(lib, d, name, C, L, v2, cf, dev="cuda:0"):
    """grad_loc (and grad_w) of one case through rac_msmv_bwd / rac_msmv_v2_bwd of `lib`"""
    vp, i = ctypes.c_void_p, ctypes.c_int
    feats = [torch.from_numpy(d[f"c{C}_feat{l}"]).to(dev) for l in range(L)]
    if cf:
        feats = [f.permute(0, 4, 1, 2, 3).contiguous() for f in feats]
    loc = torch.from_numpy(d["loc"]).to(dev)
    w = torch.from_numpy(np.ascontiguousarray(d["w"][..., :L])).to(dev)
    gout = torch.from_numpy(d[f"c{C}_gout"]).to(dev)
    gfeat = [torch.zeros_like(f) for f in feats]
    gloc = torch.empty_like(loc)
    gw = torch.empty_like(w)
    ptrs = (vp * L)(*[f.data_ptr() for f in feats])
    gptrs = (vp * L)(*[g.data_ptr() for g in gfeat])
    hw = (ctypes.c_int32 * (2 * L))(*[x for h_w in HWS[:L] for x in h_w])
    P_ = lambda t: vp(t.data_ptr())  # noqa: E731
    if v2:
        fn = lib.rac_msmv_v2_bwd
        fn.restype, fn.argtypes = i, [vp, vp, vp, i, vp, vp, vp, vp] + [i] * 6 + [vp]
        rc = fn(P_(gout), ptrs, hw, L, P_(loc), P_(w), gptrs, P_(gloc), S, N, Q, P, C, int(cf), None)
    else:
        fn = lib.rac_msmv_bwd
        fn.restype, fn.argtypes = i, [vp, vp, vp, i, vp, vp, vp, vp, vp] + [i] * 5 + [vp]
        rc = fn(P_(gout), ptrs, hw, L, P_(loc), P_(w), gptrs, P_(gloc), P_(gw), S, N, Q, P, C, None)
    assert rc == 0, name
    torch.cuda.synchronize()
    return gloc.cpu().numpy(), (None if v2 else gw.cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "msmv_bwd_pin.npz"))
    args = ap.parse_args()
    lib = ctypes.CDLL(os.path.abspath(args.lib))
    d = inputs()
    for name, C, L, v2, cf in CASES:
        gloc, gw = run_old(lib, d, name, C, L, v2, cf)
        d[name + "_gloc"] = gloc
        if gw is not None:
            d[name + "_gw"] = gw
    np.savez_compressed(args.out, **d)
    print(f"wrote {args.out}: {os.path.getsize(args.out) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
