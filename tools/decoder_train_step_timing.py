#!/usr/bin/env python3
"""Time the decoder under autograd at the f8 shape (B = 1, Q = 900, T = 8, 6 cameras, 4 levels, six layers):
  * one forward + backward of RaCFormerTransformer through the training route of the layer (forward_train), every parameter,
    the queries, both BEV map stacks and the un-regrouped pyramid requiring grad; the no_grad forward (the fused plan) for scale;
  * rac_regroup_multi_bwd alone (all levels, one launch) against torch's permute().contiguous() of the same gradients, level by
    level, and the per-level share of the kernel measured as a one-level launch.
Host-synchronised HIP events; batches alternate between the candidates so that clock and neighbours drift
alike for all.  Writes one JSON record (default profiles/decoder_train_step_f8.json).  No time is asserted anywhere.
    python tools/decoder_train_step_timing.py [--out PATH] [--rounds 4] [--batch 3] [--library-conv-grad]
                                              [--library-mixing-linears | --fused-mixing-linears]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from racformer_amd import synthetic as syn  # noqa: E402
from racformer_amd import transformer as T  # noqa: E402
from racformer_amd.fused import regroup_backward  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decoder_train_step_f8.json"))
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--library-conv-grad", action="store_true",
                    help="the temporal-fusion convolution on the library's nn.Conv2d under autograd (RadarBEVTemporalEncoder.fused_conv_grad = False)")
    ap.add_argument("--library-mixing-linears", action="store_true",
                    help="the mixing's parameter_generator and out_proj on the library's GEMMs under autograd (AdaptiveMixing.fused_linear_grad = False)")
    ap.add_argument("--fused-mixing-linears", action="store_true",
                    help="the same two Linears through _SplitLinearCore (AdaptiveMixing.fused_linear_grad = True), whatever the class default")
    ap.add_argument("--alternate-mixing-linears", metavar="PATH", default="",
                    help="also time the OTHER setting of AdaptiveMixing.fused_linear_grad, step by step in alternation with the chosen one in this "
                         "process (clock, neighbours and host load drift alike for both), and write its record to PATH")
    a = ap.parse_args()
    if a.library_conv_grad:
        T.RadarBEVTemporalEncoder.fused_conv_grad = False
    if a.library_mixing_linears or a.fused_mixing_linears:
        assert not (a.library_mixing_linears and a.fused_mixing_linears)
        T.AdaptiveMixing.fused_linear_grad = bool(a.fused_mixing_linears)
    assert torch.cuda.is_available(), "needs the MI355X: a CPU run cannot give a time"
    dev = "cuda:0"
    cfg = syn.F8
    tr = T.RaCFormerTransformer(**cfg.transformer_kwargs()).eval()
    syn.fill_params(tr, 22)
    tr = tr.to(dev)
    qb, qf = (x.to(dev) for x in syn.make_queries(cfg, 21))
    pyramid = [f.to(dev) for f in syn.make_pyramid(cfg, 21)]
    lss, radar = syn.make_bev(cfg, 21, 0).to(dev), syn.make_bev(cfg, 21, 1).to(dev)
    metas = syn.make_img_metas(cfg)
    leaves = [qb, qf, lss, radar, *pyramid]
    dims = (cfg.batch, cfg.num_frames, cfg.num_cams, cfg.channels)
    G = cfg.num_groups
    gouts = [torch.randn(cfg.batch * cfg.num_frames * G, cfg.num_cams, f.shape[3], f.shape[4], cfg.channels, device=dev) for f in pyramid]

    def torch_regroup_bwd(g):
        B, Tn, N, C = dims
        return g.view(B, Tn, G, N, g.shape[2], g.shape[3], C).permute(0, 1, 3, 2, 6, 4, 5).contiguous()

    def step():
        for x in leaves:
            x.requires_grad_(True)
        cls, box = tr(qb, qf, list(pyramid), lss, radar, None, metas)
        return cls, box

    def infer():
        with torch.no_grad():
            return tr(qb.detach(), qf.detach(), [f.detach() for f in pyramid], lss.detach(), radar.detach(), None, metas)

    g1 = g2 = None
    chosen = bool(T.AdaptiveMixing.fused_linear_grad)
    other_times, other_peak = dict(train_forward=[], train_backward=[]), 0
    times = {k: [] for k in ("train_forward", "train_backward", "nograd_forward", "regroup_multi_bwd_all_levels", "torch_permute_contiguous_all_levels")}
    per_level = {f"level{l}": dict(kernel=[], torch=[]) for l in range(len(pyramid))}
    for r in range(a.rounds + 1):                     # round 0 warms every shape up and is dropped
        fw, bw, nf, rk, rt = [], [], [], [], []
        ofw, obw = [], []
        lv = {k: dict(kernel=[], torch=[]) for k in per_level}
        for _ in range(a.batch):
            if a.alternate_mixing_linears:          # the other route first, then the chosen one: one pair per step
                T.AdaptiveMixing.fused_linear_grad = not chosen
                torch.cuda.reset_peak_memory_stats()
                t_f, (cls, box) = timed(step)
                if g1 is None:
                    g1, g2 = torch.randn_like(cls), torch.randn_like(box)
                t_b, _ = timed(lambda: ((cls * g1).sum() + (box * g2).sum()).backward())
                other_peak = torch.cuda.max_memory_allocated()
                for x in leaves:
                    x.grad = None
                tr.zero_grad(set_to_none=True)
                del cls, box
                ofw.append(t_f)
                obw.append(t_b)
                T.AdaptiveMixing.fused_linear_grad = chosen
            torch.cuda.reset_peak_memory_stats()
            t_f, (cls, box) = timed(step)
            if g1 is None:
                g1, g2 = torch.randn_like(cls), torch.randn_like(box)
            t_b, _ = timed(lambda: ((cls * g1).sum() + (box * g2).sum()).backward())
            peak = torch.cuda.max_memory_allocated()
            for x in leaves:
                x.grad = None
            tr.zero_grad(set_to_none=True)
            del cls, box
            nf.append(timed(infer)[0])
            fw.append(t_f)
            bw.append(t_b)
            rk.append(timed(lambda: regroup_backward(gouts, dims, G))[0])
            rt.append(timed(lambda: [torch_regroup_bwd(g) for g in gouts])[0])
            for l, g in enumerate(gouts):
                lv[f"level{l}"]["kernel"].append(timed(lambda: regroup_backward([g], dims, G))[0])
                lv[f"level{l}"]["torch"].append(timed(lambda: torch_regroup_bwd(g))[0])
        if r and a.alternate_mixing_linears:
            other_times["train_forward"].append(float(np.median(ofw)))
            other_times["train_backward"].append(float(np.median(obw)))
        if r:
            for k, v in (("train_forward", fw), ("train_backward", bw), ("nograd_forward", nf), ("regroup_multi_bwd_all_levels", rk),
                         ("torch_permute_contiguous_all_levels", rt)):
                times[k].append(float(np.median(v)))
            for k in per_level:
                for w in ("kernel", "torch"):
                    per_level[k][w].append(float(np.median(lv[k][w])))
    stat = lambda v: dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))   # noqa: E731
    nbytes = sum(g.numel() * 4 for g in gouts)
    rec = dict(shape=dict(B=cfg.batch, Q=cfg.num_query, T=cfg.num_frames, N=cfg.num_cams, G=G, C=cfg.channels, layers=cfg.num_layers,
                          levels=[list(f.shape[3:]) for f in pyramid], pyramid_bytes=nbytes),
               method=f"{a.rounds} rounds of alternating batches of {a.batch} after one warm-up round; host-synchronised HIP event pairs "
                      "around each candidate (allocation of the results included on both sides); microseconds",
               us={k: stat(v) for k, v in times.items()},
               regroup_bwd_per_level_us={k: dict(kernel_one_level_launch=stat(v["kernel"]), torch_permute_contiguous=stat(v["torch"]))
                                         for k, v in per_level.items()},
               fused_conv_grad=bool(T.RadarBEVTemporalEncoder.fused_conv_grad),
               fused_linear_grad=bool(T.AdaptiveMixing.fused_linear_grad),
               train_step_us_per_round=[f + b for f, b in zip(times["train_forward"], times["train_backward"])],
               train_step_peak_memory_MB=round(peak / 1e6, 1),
               device=torch.cuda.get_device_name(0))
    k_us = rec["us"]["regroup_multi_bwd_all_levels"]["median"]
    rec["regroup_multi_bwd_TBps"] = 2 * nbytes / (k_us * 1e-6) / 1e12
    rec["regroup_speedup_over_torch"] = rec["us"]["torch_permute_contiguous_all_levels"]["median"] / k_us
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.alternate_mixing_linears:
        note = ("train_forward / train_backward of fused_linear_grad = %s and = %s were timed step by step in alternation in one process; "
                "the other figures belong to the process as a whole" % (chosen, not chosen))
        rec["alternated_with"] = note
        other = dict(rec, fused_linear_grad=not chosen, train_step_peak_memory_MB=round(other_peak / 1e6, 1),
                     train_step_us_per_round=[f + b for f, b in zip(other_times["train_forward"], other_times["train_backward"])],
                     us=dict(rec["us"], **{k: stat(v) for k, v in other_times.items()}))
        with open(a.alternate_mixing_linears, "w") as f:
            json.dump(other, f, indent=1)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(dict(us=rec["us"], regroup_multi_bwd_TBps=rec["regroup_multi_bwd_TBps"],
                          regroup_speedup_over_torch=rec["regroup_speedup_over_torch"]), indent=1))


if __name__ == "__main__":
    main()
