#!/usr/bin/env python3
"""Timing of the image backbone (racformer_amd/resnet.py) on the f8 shapes: 48 images (8 frames x 6 cameras) of 3 x 256 x 704, and 6
images, the online case.  Needs the GPU.

    python tools/resnet_bench.py [--out profiles/resnet_f8.json] [--errors resnet_errors.json] [--images 48 6]

Images are [0, 255]-like BGR values with ``input_norm`` set (the stem normalises while it stages them).  Routes on the same device,
weights and inputs, alternating inside every repetition after a warm-up; medians (and the 10th / 90th percentiles: the run-to-run
spread) of device-event times in microseconds:
  stem and per stage   hip (the kernels of csrc/resnet.hip, eager) beside torch (``fused=False``: the library's convolutions, batch norm
                       and pool), each on the HIP route's own input of that stage; algorithmic bytes (every convolution's input and
                       residual read and output written once, fp32, plus the per-image-maximum passes counted separately), the
                       arithmetic in MAC, the executed FLOP (three f16 products per MAC in the stages, one fp32 fma in the stem),
                       achieved TFLOP/s and GB/s
  whole forward        hip_eager, hip_graph (one captured graph) and torch_eager
--grad: forward + backward instead (``ResNet(50, frozen_stages=1)`` in ``train()``, one random output gradient per stage), with
``fused_grad`` on and off on the same model and inputs, and the peak allocated memory of either route; the weights do not change between
the repetitions, so the once-per-weight-version packing (and its read-back of the weight maximum) is not in these times.  --errors then
names the figures a `RAC_RESNET_GRAD_ERRORS=<file> pytest -m gpu tests/test_resnet_grad_gpu.py` session wrote; they are copied into the
record.
    python tools/resnet_bench.py --grad --images 48 --out profiles/resnet_grad_f8.json [--errors resnet_grad_errors.json]
--errors (without --grad): the (E_ref, err) pairs a `RAC_RESNET_ERRORS=<file> pytest -m gpu tests/test_resnet_gpu.py` session wrote; their largest
err / E_ref per group goes into the record.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from racformer_amd import _lib, resnet  # noqa: E402

H, W = 256, 704
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def timed(fns, reps, warmup=3):
    """{name: {median, p10, p90} us}; the functions alternate inside every repetition"""
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
    out = {}
    for k, v in ev.items():
        t = sorted(1e3 * a.elapsed_time(b) for a, b in v)
        out[k] = dict(median=round(statistics.median(t), 1), p10=round(t[len(t) // 10], 1), p90=round(t[(9 * len(t)) // 10], 1))
    return out


def fill(m, gen):
    """He-normal convolutions; BatchNorm weight in [0.5, 1.5] (halved for bn3), small bias and mean, variance in [0.5, 1.5]."""
    with torch.no_grad():
        for name, mod in m.named_modules():
            if isinstance(mod, torch.nn.Conv2d):
                mod.weight.copy_(torch.randn(mod.weight.shape, generator=gen) * (2.0 / mod.weight[0].numel()) ** 0.5)
            elif isinstance(mod, torch.nn.BatchNorm2d):
                c = mod.weight.shape
                mod.weight.copy_((torch.rand(c, generator=gen) + 0.5) * (0.5 if name.endswith("bn3") else 1.0))
                mod.bias.copy_(torch.randn(c, generator=gen) * 0.1)
                mod.running_mean.copy_(torch.randn(c, generator=gen) * 0.1)
                mod.running_var.copy_(torch.rand(c, generator=gen) + 0.5)


def graph_of(step):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    return graph, captured


def stage_work(m, i, n, h, w):
    """Arithmetic and algorithmic traffic of stage i on n maps of h x w, from the layer shapes."""
    mac = act_bytes = amax_bytes = launches = 0
    for blk in getattr(m, m.res_layers[i]):
        ho, wo = resnet.conv_out_size(h, w, 3, blk.stride)
        cin, p, cout = blk.inplanes, blk.planes, blk.planes * resnet.EXPANSION
        convs = [(cin, p, 1, h * w, h * w, 0), (p, p, 9, h * w, ho * wo, 0), (p, cout, 1, ho * wo, ho * wo, cout * ho * wo)]
        if blk.downsample is not None:
            convs.append((cin, cout, 1, h * w, ho * wo, 0))
        for ci, co, taps, pin, pout, res in convs:
            mac += n * co * ci * taps * pout
            act_bytes += 4 * n * (ci * pin + co * pout + res)
        amax_bytes += 4 * n * (cin * h * w + p * h * w + p * ho * wo)
        launches += len(convs) + 3
        h, w = ho, wo
    return dict(mac=mac, algorithmic_bytes=act_bytes, absmax_pass_bytes=amax_bytes, launches=launches, executed_flop=6 * mac), (h, w)


def rates(work, t_us):
    work["achieved_TFLOPs_executed"] = round(work["executed_flop"] / (t_us * 1e-6) / 1e12, 1)
    work["achieved_GBps_algorithmic"] = round((work["algorithmic_bytes"] + work.get("absmax_pass_bytes", 0)) / (t_us * 1e-6) / 1e9, 1)


def bench(images, reps, dev):
    gen = torch.Generator().manual_seed(9)
    m = resnet.ResNet(50).eval()
    fill(m, gen)
    m = m.to(dev)
    lib = resnet.ResNet(50, fused=False).eval().to(dev)
    lib.load_state_dict(m.state_dict())
    m.input_norm = lib.input_norm = NORM
    x = (torch.rand(images, 3, H, W, generator=gen) * 255.0).to(dev)

    def hip_step():
        with torch.no_grad():
            return m(x)

    def torch_step():
        with torch.no_grad():
            return lib(x)

    with torch.no_grad():
        assert m.hip_route(x) and not lib.hip_route(x)
    ours, theirs = hip_step(), torch_step()
    torch.cuda.synchronize()
    diffs = [dict(max_abs_diff=float((a - b).abs().max()), output_max_abs=float(b.abs().max())) for a, b in zip(ours, theirs)]
    graph, captured = graph_of(hip_step)
    same = all(torch.equal(a, b) for a, b in zip(captured, ours))
    whole = timed({"hip_eager": hip_step, "hip_graph": graph.replay, "torch_eager": torch_step}, reps)

    # stem and stages alone, each on the HIP route's own input of that stage (copies: the scratch they come from is reused)
    with torch.no_grad():
        ins = [m.stem_hip(x).clone()]
        for i in range(3):
            ins.append(m.stage_hip(i, ins[-1]).clone())
    (hc, wc), (hp, wp) = resnet.stem_sizes(H, W)
    stem_mac = images * 64 * 147 * hc * wc
    rows = {"stem": dict(mac=stem_mac, executed_flop=2 * stem_mac, launches=2,
                         algorithmic_bytes=4 * images * (3 * H * W + 64 * hp * wp),
                         conv_output_round_trip_bytes=2 * 4 * images * 64 * hc * wc)}
    fns = {}

    def no_grad(f):
        def g():
            with torch.no_grad():
                return f()
        return g

    fns["stem:hip"] = no_grad(lambda: m.stem_hip(x))
    fns["stem:torch"] = no_grad(lambda: lib.maxpool(lib.relu(lib.bn1(lib.conv1(resnet.apply_input_norm(x, NORM))))))
    h, w = hp, wp
    for i in range(4):
        rows[f"layer{i + 1}"], (h2, w2) = stage_work(m, i, images, h, w)
        rows[f"layer{i + 1}"]["map_in"] = [h, w]
        fns[f"layer{i + 1}:hip"] = no_grad(lambda i=i: m.stage_hip(i, ins[i]))
        fns[f"layer{i + 1}:torch"] = no_grad(lambda i=i: getattr(lib, f"layer{i + 1}")(ins[i]))
        h, w = h2, w2
    t = timed(fns, reps)
    for k, r in rows.items():
        r["hip"], r["torch"] = t[f"{k}:hip"], t[f"{k}:torch"]
        rates(r, r["hip"]["median"])
    total_mac = sum(r["mac"] for r in rows.values())
    return dict(images=images, whole_forward=whole, graph_replay_equals_eager_bitwise=bool(same), hip_vs_torch_route=diffs,
                total_GMAC=round(total_mac / 1e9, 1), total_algorithmic_GB=round(sum(r["algorithmic_bytes"] for r in rows.values()) / 1e9, 2),
                parts=rows)


def bench_grad(images, reps, dev):
    """Forward + backward of ResNet(50, frozen_stages=1) in train() with ``fused_grad`` on and off: one model, weights, inputs and one
    random output gradient per stage; the routes alternate inside every repetition.  Rows: the whole step, and the step with only the
    last one, two and three stages trainable (the forward is the same in all: the increments are what a stage's backward costs)."""
    gen = torch.Generator().manual_seed(9)
    m = resnet.ResNet(50, frozen_stages=1, norm_eval=True)
    fill(m, gen)
    m = m.to(dev).train()
    m.input_norm = NORM
    x = (torch.rand(images, 3, H, W, generator=gen) * 255.0).to(dev)
    with torch.no_grad():
        shapes = [tuple(o.shape) for o in m(x)]
    gouts = [torch.randn(s, generator=gen).to(dev) for s in shapes]

    def trainable_from(stage):
        for i, name in enumerate(m.res_layers):
            for p in getattr(m, name).parameters():
                p.requires_grad_(i >= stage)

    def step(switch, stage):
        def run():
            m.fused_grad = switch
            trainable_from(stage)
            for p in m.parameters():
                p.grad = None
            assert m.hip_grad_route(x) == switch
            outs = m(x)
            pairs = [(o, g) for o, g in zip(outs, gouts) if o.requires_grad]
            torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])
        return run

    rows, fns = {}, {}
    for stage in (1, 2, 3):
        key = "layer%d..4" % (stage + 1) if stage < 3 else "layer4"
        fns[f"{key}:hip"], fns[f"{key}:torch"] = step(True, stage), step(False, stage)
    t = timed(fns, reps, warmup=2)
    peak = {}
    for route, switch in (("hip", True), ("torch", False)):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        step(switch, 1)()
        torch.cuda.synchronize()
        peak[route] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)
    for key in ("layer4", "layer3..4", "layer2..4"):
        rows[key] = dict(hip=t[f"{key}:hip"], torch=t[f"{key}:torch"],
                         faster="hip" if t[f"{key}:hip"]["median"] < t[f"{key}:torch"]["median"] else "torch")
    inc = {}
    for name, a, b in (("layer4", "layer4", None), ("layer3", "layer3..4", "layer4"), ("layer2", "layer2..4", "layer3..4")):
        d = {r: round(rows[a][r]["median"] - (rows[b][r]["median"] if b else 0.0), 1) for r in ("hip", "torch")}
        d["faster"] = "hip" if d["hip"] < d["torch"] else "torch"
        inc[name] = d
    return dict(images=images, forward_plus_backward=rows, increment_per_stage=inc, peak_allocated_GiB=peak,
                note="increment_per_stage: layer4 = the step with only layer4 trainable (it contains the whole forward), layer3 and "
                     "layer2 = what making that stage trainable as well adds (its backward and the tensors it keeps)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "resnet_f8.json"))
    ap.add_argument("--errors", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--images", type=int, nargs="+", default=[48, 6])
    ap.add_argument("--grad", action="store_true", help="forward + backward with fused_grad on and off (profiles/resnet_grad_f8.json)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resnet_bench needs the MI355X"
    _lib.lib()
    if args.grad:
        rec = dict(shape=dict(image=[3, H, W], depth=50, frozen_stages=1, norm_eval=True, input_norm=NORM),
                   device=torch.cuda.get_device_name(0), unit="us: median, 10th and 90th percentile of device-event times",
                   reps=args.reps, runs=[bench_grad(n, args.reps, "cuda:0") for n in args.images])
        if args.errors and os.path.exists(args.errors):
            rec["test_figures"] = json.load(open(args.errors))
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
        print(json.dumps({k: v for k, v in rec.items() if k != "test_figures"}, indent=1))
        return
    rec = dict(shape=dict(image=[3, H, W], depth=50, input_norm=NORM), device=torch.cuda.get_device_name(0),
               unit="us: median, 10th and 90th percentile of device-event times", reps=args.reps,
               runs=[bench(n, args.reps, "cuda:0") for n in args.images])
    rec["derived_not_measured"] = [
        "mac, algorithmic_bytes, absmax_pass_bytes and executed_flop come from the layer shapes",
        "no counter was read: how much of the repeated reads (every channel block of a convolution re-reads its pixel tile; the 3x3 reads "
        "each pixel nine times) is served by L2 / the Infinity Cache is not known",
    ]
    rec["open_work"] = [
        "the per-image maximum is a pass of its own over every convolution input (absmax_pass_bytes): writing tile maxima from the "
        "producing convolution's epilogue would remove it",
        "every channel block of a convolution re-splits its pixel tile's operands: an f16 hi/lo activation image between the layers of "
        "a block would split each value once",
        "the stem writes and re-reads its convolution output (conv_output_round_trip_bytes) between its two launches: pooling in the "
        "convolution's workgroup would remove the round trip",
        "fusing a whole Bottleneck into one kernel; writing the necks' operands from the last block's epilogue",
    ]
    if args.errors and os.path.exists(args.errors):
        pairs = json.load(open(args.errors))
        worst = {}
        for p in pairs:
            ratio = p["err"] / p["e_ref"] if p["e_ref"] > 0 else float("inf")
            rel = p["err"] / p["want_max"] if p["want_max"] > 0 else 0.0
            g = worst.setdefault(p["group"], dict(cases=0, max_err_over_e_ref=0.0, max_err_over_want_max=0.0, needs_relative_term=0))
            g["cases"] += 1
            if ratio > g["max_err_over_e_ref"]:
                g["max_err_over_e_ref"], g["worst_case"] = round(ratio, 2), p["case"]
            g["max_err_over_want_max"] = max(g["max_err_over_want_max"], float(f"{rel:.3e}"))
            g["needs_relative_term"] += int(p["err"] >= p["stages"] * (4 * p["e_ref"] + 1e-6))
        rec["tolerance_groups"] = worst
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
