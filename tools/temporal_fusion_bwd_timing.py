#!/usr/bin/env python3
"""Time the temporal-fusion convolution under autograd at the f8 shape (N = 8 frames, 128 x 128, 320 -> 256, 3x3):
  * the library route: F.conv2d of cat[x, hid] forward and its backward (all four gradients), under
    cudnn.flags(deterministic=True) as prepare_train sets it;
  * the HIP route (_TemporalFusionCore) forward and backward as autograd runs them, and its pieces alone: the forward (scale, two
    packs, rac_conv3x3_fwd), the image of the output gradient (scale + channel-last pack), the data-gradient launch of x, the one
    of the hidden half (zero-padded weight image), the re-pack of the input image, rac_conv3x3_wgrad (both of its launches) and
    the bias sum;
  * the three weight packs (forward image, transposed images of the x and hidden halves: torch ops and one host
    synchronisation each), which a step whose weights changed pays once and the figures above do NOT contain -- they are taken
    with unchanged weights, packed in the warm-up round.  Wall clock between two device synchronisations, because the cost is
    the host's wait as much as the device's work.
Host-synchronised HIP events; batches alternate between the candidates so that clock and neighbours drift alike for all.
Writes one JSON record (default profiles/temporal_fusion_bwd_f8.json).  No time is asserted anywhere.
    python tools/temporal_fusion_bwd_timing.py [--out PATH] [--rounds 4] [--batch 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from racformer_amd import fused  # noqa: E402
from racformer_amd import transformer as T  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_fusion_bwd_f8.json"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--shape", type=int, nargs=4, default=[8, 128, 128, 64], metavar=("N", "H", "W", "HIDDEN"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run cannot give a time"
    dev = "cuda:0"
    N, H, W, hd = a.shape
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, 256, H, W, generator=g).to(dev).requires_grad_()
    hid = (torch.randn(N, hd, H, W, generator=g) * 0.5).to(dev).requires_grad_()
    w = (torch.randn(256, 256 + hd, 3, 3, generator=g) * 0.03).to(dev).requires_grad_()
    b = (torch.randn(256, generator=g) * 0.1).to(dev).requires_grad_()
    gy_cl = torch.randn(N, H, W, 256, generator=g).to(dev)          # channel-last, as the HIP route's consumer hands it over
    gy = gy_cl.permute(0, 3, 1, 2).contiguous()                    # the same values channel-first, as the library route's consumer does
    leaves = (x, hid, w, b)
    ws, alpha = fused.pack_conv3x3_weight(w)
    packs = dict(ws=ws, alpha=alpha)

    def clear():
        for t in leaves:
            t.grad = None

    def lib_fwd():
        with torch.backends.cudnn.flags(enabled=True, deterministic=True):
            return F.conv2d(torch.cat([x, hid], dim=1), w, b, padding=1)

    def lib_bwd(out):
        with torch.backends.cudnn.flags(enabled=True, deterministic=True):
            out.backward(gy)

    def hip_fwd():
        return T._TemporalFusionCore.apply(x, hid, w, b, packs)

    xd, hd_, wd = x.detach(), hid.detach(), w.detach()
    g_img = fused.ConvImage(N, H, W, 256, dev)
    x_img = fused.ConvImage(N, H, W, 256 + hd, dev)
    pieces = dict(
        hip_forward_alone=lambda: fused.temporal_fusion_forward(xd, hd_, ws, alpha, b.detach()),
        grad_image=lambda: g_img.begin([gy_cl]).pack_cl(gy_cl, 0),
        dgrad_x=lambda: g_img.conv(*packs["dx"][:2]),
        dgrad_hid_zero_padded=lambda: g_img.conv(*packs["dh"][:2]),
        input_image=lambda: x_img.begin([xd, hd_]).pack(xd, 0).pack(hd_, 256),
        wgrad=lambda: fused.conv3x3_wgrad(x_img, g_img),
        bias_sum=lambda: gy_cl.sum(dim=(0, 1, 2)),
    )
    def weight_packs():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fused.pack_conv3x3_weight(wd)
        fused.pack_conv3x3_dgrad_weight(wd, 0)
        fused.pack_conv3x3_dgrad_weight(wd, 256)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    keys = ["library_forward", "library_backward", "hip_forward", "hip_backward", *pieces, "weight_packs_wall"]
    times = {k: [] for k in keys}
    for r in range(a.rounds + 1):                     # round 0 warms every shape up (and packs the transposed weights) and is dropped
        cur = {k: [] for k in keys}
        for _ in range(a.batch):
            t, out = timed(lib_fwd)
            cur["library_forward"].append(t)
            cur["library_backward"].append(timed(lambda: lib_bwd(out))[0])
            clear()
            del out
            t, out = timed(hip_fwd)
            cur["hip_forward"].append(t)
            cur["hip_backward"].append(timed(lambda: out.backward(gy_cl))[0])
            clear()
            del out
            for k, fn in pieces.items():
                cur[k].append(timed(fn)[0])
            cur["weight_packs_wall"].append(weight_packs())
        if r:
            for k in keys:
                times[k].append(float(np.median(cur[k])))
    stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))   # noqa: E731
    rec = dict(shape=dict(N=N, H=H, W=W, Cin=256 + hd, Cout=256, k_splits=fused.wgrad_k_splits(N, H, W, 256 + hd)),
               method=f"{a.rounds} rounds of alternating batches of {a.batch} after one warm-up round; host-synchronised HIP event pairs "
                      "around each candidate (allocation of the results included on all sides); per round the median of the batch; "
                      "median / min / max over the rounds; microseconds.  hip_forward / hip_backward and the pieces hold for UNCHANGED weights "
                      "(packed in the warm-up round); weight_packs_wall is what a step whose weights changed adds once: the three packs, "
                      "host wall clock between two device synchronisations",
               us={k: stat(v) for k, v in times.items()},
               device=torch.cuda.get_device_name(0))
    lb, hb = rec["us"]["library_backward"], rec["us"]["hip_backward"]
    pk = rec["us"]["weight_packs_wall"]
    rec["backward_speedup_over_library"] = lb["median"] / hb["median"]
    rec["backward_faster_beyond_round_spread"] = bool(hb["max"] < lb["min"])
    rec["backward_plus_packs_faster_beyond_round_spread"] = bool(hb["max"] + pk["max"] < lb["min"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
