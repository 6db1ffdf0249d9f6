#!/usr/bin/env python3
"""Pin of the single-writer outputs of rac_bev_sampling_bwd / rac_bev_sampling_bwd_batch as a given build of libracformer_hip.so
computes them (MI355X only).  Writes bev_bwd_pin.npz: per case the seed and dims, a float64 checksum of every drawn input (so that a
drifted draw is told apart from a changed kernel) and grad_offsets, grad_ray, grad_scale, grad_queue, grad_box and the debug outputs
grad_loc, grad_attn -- not the inputs, which ``draw`` redraws with case(...) of tests/test_bev_sampling_batch_grad_cpu.py, and not
grad_value (float atomics, sums in arrival order).  The cases are the smallest that enter every loop's second trip; the B = 1 ones go
through both symbols, which must agree to the bit (one copy is stored).  tests/test_bev_sampling_batch_grad_gpu.py checks that the
current build returns the pinned tensors bit for bit.

The library is loaded on its own (not through racformer_amd._lib), so the pin can be made with a build of another commit:
    python tests/golden/gen_bev_bwd_pin.py --lib path/to/libracformer_hip.so [--out tests/golden/bev_bwd_pin.npz]
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
from test_bev_sampling_batch_grad_cpu import case  # noqa: E402

# name -> (seed, B, T, Q, heads, NP, D, H, W, queries beyond the map, smallest query radius / 65 m)
CASES = {
    "B1 T1 h1 P7 16x16": (33, 1, 1, 6, 1, 7, 1, 16, 16, False, 0.05),
    "B1 T3 h4 P10 12x10": (31, 1, 3, 9, 4, 2, 5, 12, 10, False, 0.05),
    "B1 T8 h4 P20 128x128": (32, 1, 8, 12, 4, 4, 5, 128, 128, False, 0.05),      # 640 keypoints: three trips of the 256-strided loops
    "B2 T3 h4 P10 12x10": (21, 2, 3, 6, 4, 2, 5, 12, 10, False, 0.05),
    "B3 T4 h1 P3 8x8": (22, 3, 4, 6, 1, 1, 3, 8, 8, False, 0.05),
    "B4 T2 h1 P10 12x10 beyond": (24, 4, 2, 6, 1, 2, 5, 12, 10, True, 0.05),    # clamped locations
    "B4 T8 h4 P20 16x16 77KB": (26, 4, 8, 6, 4, 4, 5, 16, 16, False, 0.3),       # B*heads*P = 320 > 256; the raised dynamic-LDS limit
}
INPUTS = ("value", "query_bbox", "off", "ray", "sc", "qu", "time_diff")
OUTPUTS = ("offsets", "ray", "scale", "queue", "box", "loc", "attn")


def symbols(name):
    """whether each entry point takes the case: (False: rac_bev_sampling_bwd, True: rac_bev_sampling_bwd_batch)"""
    return (False, True) if CASES[name][1] == 1 else (True,)


def draw(name):
    *dims, outside, d_lo = CASES[name]
    return case(*dims, outside=outside, dtype=np.float32, d_lo=d_lo)


def checksums(c, gout):
    return np.array([float(c[k].double().sum()) for k in INPUTS] + [float(gout.double().sum())])


def run(lib, c, gout, batch, dev="cuda:0"):
    """OUTPUTS of one case through rac_bev_sampling_bwd (batch = False) or rac_bev_sampling_bwd_batch of `lib`, the box table from
    its rac_box_prep_fwd"""
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    P_ = lambda t: vp(t.data_ptr())  # noqa: E731
    g = {k: c[k].to(dev).contiguous() for k in INPUTS}
    gout = gout.to(dev).contiguous()
    B, Q, _ = g["query_bbox"].shape
    T, Hn, NP, D, (H, W) = c["T"], c["heads"], c["NP"], c["D"], c["hw"]
    P = NP * D
    new = lambda *shape: torch.empty(*shape, device=dev, dtype=torch.float32)  # noqa: E731
    pc = (f * 6)(*[float(v) for v in c["pc"]])
    table = new(B, Q, 8)
    lib.rac_box_prep_fwd.restype, lib.rac_box_prep_fwd.argtypes = i, [vp, vp, i, vp, vp]
    assert lib.rac_box_prep_fwd(P_(g["query_bbox"]), P_(table), B * Q, pc, None) == 0
    out = dict(value=torch.zeros_like(g["value"]), offsets=new(B, Q, Hn * P * 2), ray=new(B, Q, D), scale=new(B, Q, Hn * P),
               queue=new(B, Q, T), box=new(B, Q, 8), loc=new(B, Q, Hn, T, P, 2), attn=new(B, Q, Hn, T, P))
    dbase = (f * D)(*torch.linspace(-c["d_region"], c["d_region"], D).tolist())
    fn = lib.rac_bev_sampling_bwd_batch if batch else lib.rac_bev_sampling_bwd
    fn.restype, fn.argtypes = i, [vp] * 17 + [i] * 17 + [vp, vp, f, i, vp]
    ld = (Hn * P * 2, D, Hn * P, T)
    rc = fn(P_(g["value"]), P_(g["query_bbox"]), P_(table), P_(g["off"]), P_(g["ray"]), P_(g["sc"]), P_(g["qu"]), P_(g["time_diff"]),
            P_(gout), *[P_(out[k]) for k in ("value",) + OUTPUTS], *ld, *ld, B, T, Q, Hn, NP, D, H, W, 64, pc, dbase, c["d_region"], 0,
            None)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in OUTPUTS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default=os.path.join(HERE, "bev_bwd_pin.npz"))
    args = ap.parse_args()
    lib = ctypes.CDLL(os.path.abspath(args.lib))
    d = {}
    for name in CASES:
        c, gout = draw(name)
        d[name + "|case"] = np.array(CASES[name], dtype=np.float64)
        d[name + "|checksums"] = checksums(c, gout)
        runs = [run(lib, c, gout, batch) for batch in symbols(name)]
        for k in OUTPUTS:
            assert np.isfinite(runs[0][k]).all() and all(np.array_equal(runs[0][k], r[k]) for r in runs[1:]), (name, k)
            d[f"{name}|grad_{k}"] = runs[0][k]
    np.savez_compressed(args.out, **d)
    print(f"wrote {args.out}: {os.path.getsize(args.out) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
