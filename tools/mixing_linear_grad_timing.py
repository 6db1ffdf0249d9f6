#!/usr/bin/env python3
"""Device-event times of AdaptiveMixing's two big Linears under autograd at the f8 shape (Q = 900, G = 4, P = 96: the generator
256 -> 65536, out_proj 32768 -> 256; B = 1 and B = 2, i.e. M = 900 and 1800 rows), split-precision route against the library:
  * every launch of the new route alone (the packs with a device-side scale, rac_generator_ds_fwd as forward and as out_proj's
    data gradient, rac_outproj_fwd + rac_linear_reduce as forward and as the generator's data gradient, rac_linear_wgrad in both
    orientations, rac_absmax_fwd over the two large operands) and the weight packs that happen once per weight version;
  * forward + backward of both Linears through _SplitLinearCore against nn.Linear + the split-K torch.bmm of
    AdaptiveMixing.forward under autograd, in alternating batches; peak memory of one such step on either route.
The mixing core between the two Linears is not part of it: Z is a leaf that requires grad.  After a warm-up the two sides of a
pair run in alternating batches, each batch between two events, until each has --window-ms of timed launches; per launch:
median / min / max over the batches.  No time is asserted anywhere.

    python tools/mixing_linear_grad_timing.py [--out profiles/mixing_linear_grad_f8.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from msmv_v2_timing import time_pair  # noqa: E402
from racformer_amd import fused as Fz  # noqa: E402
from racformer_amd import transformer as T  # noqa: E402


def stat(per_launch, total_ms):
    return {"median_us": round(statistics.median(per_launch) * 1e3, 2), "min_us": round(min(per_launch) * 1e3, 2),
            "max_us": round(max(per_launch) * 1e3, 2), "batches": len(per_launch), "timed_ms": round(total_ms, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--batch", type=int, default=5)
    ap.add_argument("--window-ms", type=float, default=120.0)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    dev = "cuda:0"
    G, P, Q = 4, 96, 900
    rec = {"what": "AdaptiveMixing's parameter_generator and out_proj under autograd at f8: the split-precision route's launches "
                   "alone, and forward + backward of both Linears on it against nn.Linear + torch.bmm (split-K) under autograd; "
                   "alternating batches of launches between device events (tools/mixing_linear_grad_timing.py)",
           "batch": args.batch, "warmup_launches_each": args.warmup, "device": torch.cuda.get_device_name(0)}
    torch.manual_seed(0)
    m = T.AdaptiveMixing(in_dim=64 * G, in_points=P, n_groups=G, query_dim=256, out_points=128).to(dev)
    with torch.no_grad():
        m.parameter_generator.weight.normal_(0, 1 / 16)       # (the model initialises it to zero, which has no image)
    gen, proj = m.parameter_generator, m.out_proj
    N, K = gen.out_features, proj.in_features

    def pair(name_a, fa, name_b, fb, into):
        res, total = time_pair(fa, fb, args.batch, args.window_ms, args.warmup)
        into[name_a], into[name_b] = stat(res["a"], total["a"]), stat(res["b"], total["b"])

    once = rec["weight_packs_per_weight_version"] = {}
    pair("pack_gemm_split_weight(generator)+(out_proj)", lambda: (Fz.pack_gemm_split_weight(gen.weight), Fz.pack_gemm_split_weight(proj.weight)),
         "pack_linear_weight_t(generator)+(out_proj)", lambda: (Fz.pack_linear_weight_t(gen.weight), Fz.pack_linear_weight_t(proj.weight)), once)
    packs = m.linear_grad_packs()
    for B in (1, 2):
        M = B * Q
        r = rec[f"B{B}"] = {"shape": {"M": M, "G": G, "P": P, "generator": [256, N], "out_proj": [K, 256], "dtype": "float32"}}
        g = torch.Generator().manual_seed(B)
        query = torch.randn(M, 256, generator=g).to(dev)
        z = torch.randn(M, K, generator=g).abs_().to(dev)
        dp = torch.randn(M, N, generator=g).to(dev)
        gy = torch.randn(M, 256, generator=g).to(dev)
        am = {k: Fz.absmax_device(v) for k, v in (("q", query), ("z", z), ("dp", dp), ("g", gy))}
        q_img, g_img = Fz.linear_pack_act(query, am["q"]), Fz.linear_pack_act(gy, am["g"])
        z_img, dp_img = Fz.linear_pack_act(z, am["z"]), Fz.linear_pack_act(dp, am["dp"])
        wt_gen, wt_out = packs.transposed("gen"), packs.transposed("out")
        params, dz = torch.empty(M, N, device=dev), torch.empty(M, K, device=dev)
        dw_out, dw_gen = torch.empty(256, K, device=dev), torch.empty(N, 256, device=dev)
        L = r["launches"] = {}
        pair("absmax(Z)", lambda: Fz.absmax_device(z), "absmax(dP)", lambda: Fz.absmax_device(dp), L)
        pair("pack_act(Z)", lambda: Fz.linear_pack_act(z, am["z"], out=z_img), "pack_act(dP)", lambda: Fz.linear_pack_act(dp, am["dp"], out=dp_img), L)
        pair("pack_act(query)", lambda: Fz.linear_pack_act(query, am["q"], out=q_img), "pack_act(g)", lambda: Fz.linear_pack_act(gy, am["g"], out=g_img), L)
        pair("generator forward (rac_generator_ds_fwd)", lambda: Fz.generator_ds(q_img, packs["gen_img"], gen.bias, packs["gen_alpha"], am["q"], out=params),
             "out_proj dZ (rac_generator_ds_fwd)", lambda: Fz.generator_ds(g_img, wt_out[0], None, wt_out[1], am["g"], out=dz), L)
        pair("out_proj forward (rac_outproj_fwd + rac_linear_reduce)",
             lambda: Fz.linear_reduce(Fz.outproj_fused(z_img, packs["out_img"], Fz.outproj_slices(K)), proj.bias, am["z"], packs["out_alpha"]),
             "generator dquery (rac_outproj_fwd + rac_linear_reduce)",
             lambda: Fz.linear_reduce(Fz.outproj_fused(dp_img, wt_gen[0], Fz.outproj_slices(N)), None, am["dp"], wt_gen[1]), L)
        pair("dW_out (rac_linear_wgrad)", lambda: Fz.linear_wgrad(g_img, am["g"], z, am["z"], False, out=dw_out),
             "dW_gen + db_gen (rac_linear_wgrad)", lambda: Fz.linear_wgrad(q_img, am["q"], dp, am["dp"], True, colsum=True, out=dw_gen), L)
        L["GFLOP"] = {"generator forward": 2e-9 * M * 256 * N, "out_proj forward": 2e-9 * M * K * 256}
        del z_img, dp_img, params, dz, dw_out, dw_gen

        qg, zg = query.clone().requires_grad_(), z.clone().requires_grad_()

        def split_step():
            p_ = T._SplitLinearCore.apply("gen", qg, gen.weight, gen.bias, packs)
            y = T._SplitLinearCore.apply("out", zg, proj.weight, proj.bias, packs)
            torch.autograd.backward([p_, y], [dp, gy])
            qg.grad = zg.grad = None
            m.zero_grad(set_to_none=True)

        def library_step():
            p_ = gen(qg)
            w3 = m.split_out_proj()
            S_, n_, k_ = w3.shape
            y = torch.bmm(zg.view(M, S_, k_).transpose(0, 1), w3.transpose(1, 2)).sum(0) + proj.bias
            torch.autograd.backward([p_, y], [dp, gy])
            qg.grad = zg.grad = None
            m.zero_grad(set_to_none=True)

        S = r["forward_and_backward_of_both_linears"] = {}
        pair("split_precision_route", split_step, "library_route", library_step, S)
        S["library_over_split_median"] = round(S["library_route"]["median_us"] / S["split_precision_route"]["median_us"], 3)
        for name, fn in (("split_precision_route", split_step), ("library_route", library_step)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            fn()
            torch.cuda.synchronize()
            S[name]["peak_memory_above_inputs_MB"] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
        del query, z, dp, gy, qg, zg, q_img, g_img
        torch.cuda.empty_cache()
    text = json.dumps(rec, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
