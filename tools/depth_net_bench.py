#!/usr/bin/env python3
"""Timing of DepthNet (racformer_amd/depth_net.py) on the f8 shape: 256 channels, D = 96, 16 x 44 feature maps, B*N = 6 maps (one
view-transform call) and B*N = 48 (eight frames batched).  Needs the GPU.

    python tools/depth_net_bench.py [--out profiles/depth_net_f8.json] [--errors depth_net_errors.json]

One step = DepthNet on the index maps of the radar priors (``forward_fused``) / on the dense priors (the torch route).  Routes on
the same device, weights and inputs, alternating inside every repetition after a warm-up; medians of device-event times in
microseconds:
  hip_eager / hip_graph   the kernels of csrc/depth_net.hip, eager and as a captured graph
  torch_eager             the module's own torch route (fused=False): the library's convolutions
Per entry point: every distinct launch of the step alone (eager, its output allocated by the call), the launches of one step and
the workgroups of each.  --errors: the (E_ref, kernel error) pairs a `RAC_DEPTH_NET_ERRORS=<file> pytest -m gpu
tests/test_depth_net_gpu.py` session wrote, copied into the record.
"""
import argparse
import collections
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from racformer_amd import depth_net as DN, lss_depth as LD  # noqa: E402

C, CONTEXT, D, H, W, E, N_RCS = 256, 256, 96, 16, 44, 32, 64


def timed(fns, reps, warmup=10):
    """{name: median us}; the functions alternate inside every repetition"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: round(1e3 * statistics.median(a.elapsed_time(b) for a, b in v), 2) for k, v in ev.items()}


def perturb(net, gen):
    """BatchNorm statistics and affine parameters away from their initial values"""
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
                m.weight.copy_(0.6 + 0.8 * torch.rand(m.weight.shape, generator=gen))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=gen))
                m.running_mean.copy_(0.2 * torch.randn(m.bias.shape, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=gen))


def bench(maps, reps, dev="cuda:0"):
    gen = torch.Generator().manual_seed(maps)
    torch.manual_seed(3)
    net = DN.DepthNet(C, C, CONTEXT, D, use_dcn=False).eval()
    perturb(net, gen)
    net = net.to(dev)
    lib_net = DN.DepthNet(C, C, CONTEXT, D, use_dcn=False, fused=False).eval().to(dev)
    lib_net.load_state_dict(net.state_dict())
    x = torch.randn(maps, C, H, W, generator=gen).to(dev)
    bins = torch.randint(0, D + 1, (maps, H, W), generator=gen, dtype=torch.int32)
    bins[torch.rand(maps, H, W, generator=gen) < 0.8] = D
    bins = bins.to(dev)
    cls = torch.randint(-1, N_RCS, (maps, H, W), generator=gen, dtype=torch.int32).to(dev)
    ew, eb = (0.3 * torch.randn(E, N_RCS, 1, 1, generator=gen)).to(dev), (0.1 * torch.randn(E, generator=gen)).to(dev)
    mlp = torch.randn(1, maps, 9, generator=gen).to(dev)
    prior = LD.radar_prior_forward(bins, cls, ew, eb, D)
    rf, re = prior[:, :D + 1].contiguous(), prior[:, D + 1:].contiguous()

    def hip_step():
        with torch.no_grad():
            return net.forward_fused(x, bins, cls, ew, eb, mlp)

    def hip_dense_step():
        with torch.no_grad():
            return net(x, rf, re, mlp)

    def torch_step():
        with torch.no_grad():
            return lib_net(x, rf, re, mlp)

    DN.trace = []
    ours = hip_step()
    launches, DN.trace = DN.trace, None
    theirs = torch_step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            hip_step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = hip_step()
    graph.replay()
    torch.cuda.synchronize()
    times = timed({"hip_eager": hip_step, "hip_graph": graph.replay, "hip_eager_dense_priors": hip_dense_step, "torch_eager": torch_step},
                  reps)

    # ---- every distinct launch alone
    pk = net.packed()
    new = lambda *s: torch.empty(*s, device=dev)                 # noqa: E731
    rows, rows4, gates, img_bias = new(maps, H * W, C), new(maps, H * W, 4 * C), torch.rand(2, maps, C, device=dev), new(maps, C)
    table = net.rcs_table(ew, eb)
    w1, b1, w2, b2 = pk["blocks"][0]
    conv = lambda *a, **k: (lambda: DN.conv_small(*a, **k))      # noqa: E731
    entry = {
        "rac_conv_small_pack_fwd(x)": lambda: DN.pack_rows(x, rows),
        "rac_depthnet_gates_fwd": lambda: DN._lib.check(DN._lib.lib().rac_depthnet_gates_fwd(
            DN._lib.ptr(mlp), DN._lib.ptr(pk["gates"]), DN._lib.ptr(gates), maps, C, 2, DN._lib.stream_ptr()), "gates"),
        "rac_depthnet_pool_bias_fwd": lambda: DN._lib.check(DN._lib.lib().rac_depthnet_pool_bias_fwd(
            DN._lib.ptr(rows), DN._lib.ptr(pk["pool"][0]), DN._lib.ptr(pk["pool"][1]), DN._lib.ptr(pk["conv1"][2]), DN._lib.ptr(img_bias),
            maps, H * W, C, C, C, DN._lib.stream_ptr()), "pool"),
        "rac_conv_small_fwd(3x3 d1 bias relu)": conv(rows, w1, C, H, W, ksize=3, bias=b1, relu=True),
        "rac_conv_small_fwd(3x3 d1 bias residual relu)": conv(rows, w2, C, H, W, ksize=3, bias=b2, residual=rows, relu=True),
        "rac_conv_small_fwd(1x1 gate -> context, channel-first)": conv(rows, pk["context"][0], CONTEXT, H, W, bias=pk["context"][1], gate=gates[0],
                                                                       channel_first=True),
        "rac_conv_small_fwd(1x1 gate + prior lookup)": conv(rows, pk["dep_x"], C, H, W, bias=pk["dep_bias"], gate=gates[1], bins=bins,
                                                            bins_table=pk["bins_table"], cls=cls, cls_table=table),
        "rac_conv_small_fwd(1x1 1024 image bias relu)": conv(rows4, pk["conv1"][0], C, H, W, bias=pk["conv1"][1], img_bias=img_bias, relu=True),
        "rac_conv_small_fwd(1x1 -> D, channel-first)": conv(rows, pk["final"][0], D, H, W, bias=pk["final"][1], channel_first=True),
    }
    for w, b, k, dil in pk["aspp"]:
        entry[f"rac_conv_small_fwd(aspp {k}x{k} d{dil} -> concat)"] = conv(rows, w, C, H, W, ksize=k, dilation=dil, bias=b, relu=True, out=rows4,
                                                                         c_off=0)
    entry_points = timed(entry, reps)
    per_entry = collections.OrderedDict()
    for name, label, wgs in launches:
        e = per_entry.setdefault(name, dict(launches=0, workgroups_per_launch=collections.OrderedDict()))
        e["launches"] += 1
        e["workgroups_per_launch"][label] = wgs
    return dict(maps=maps, pixels=maps * H * W, times=times, entry_points=entry_points,
                launches=dict(hip=len(launches), by_entry_point=per_entry, torch_device_kernels="not measured"),
                hip_vs_torch_route_max_abs_diff=float((ours - theirs).abs().max()), output_max_abs=float(theirs.abs().max()),
                graph_replay_equals_eager_bitwise=bool(torch.equal(captured, ours)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "depth_net_f8.json"))
    ap.add_argument("--errors", default=None)
    ap.add_argument("--reps", type=int, default=100)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "depth_net_bench needs the MI355X"
    rec = dict(shape=dict(channels=C, context=CONTEXT, D=D, h=H, w=W, rcs_classes=N_RCS, embedding=E),
               device=torch.cuda.get_device_name(0), unit="us, median of device-event times around one step", reps=args.reps,
               step="DepthNet.forward_fused (hip) / DepthNet.forward with fused=False on the dense priors (torch), eval, no grad",
               runs={f"maps_{m}": bench(m, args.reps) for m in (6, 48)})
    if args.errors and os.path.exists(args.errors):
        rec["tolerance_bases"] = json.load(open(args.errors))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
