#!/usr/bin/env python3
"""Golden gradients of one decoder layer: runs the REFERENCE's own RaCFormerTransformerDecoderLayer
(racformer_transformer.py:145-279) on CPU in eval mode -- every module's checkpoint wrapper is bypassed there and dropout is
off --, where msmv_sampling takes the differentiable grid_sample path and the MSDA op its torch formulation, followed by
theta_d2xy_coods of the refined boxes (:134), backpropagates sum(query_feat * g0) + sum(cls_score * g1) + sum(bbox_xy * g2) for
seeded gouts, and writes a data-only fixture next to this script.  Run in the build container only (needs the reference tree,
see ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_decoder_grad.py

  decoder_grad_small.npz (+ decoder_grad_small.1.npz: the gradients; each file below the repository's 1 MiB limit)
                        the rig of tests/decoder_grad_ref.py.  Inputs (query_bbox, query_feat, feat{l} channel-last and lss /
                        radar as float16: multiples of 1/8; time_diff, lidar2img, the three gouts), the seed of the inputs and of
                        the weights with a float64 checksum per weight (the weights are float16-exact and a function of the seed:
                        the layer has 14 M parameters, and the fixture must stay small), the outputs in float32 and, per gradient
                        tensor "g32:<name>" / "g64:<name>" (parameters as "p:<state_dict key>"): the reference's float32 and float64
                        gradients -- whole up to 2048 elements, else 1024 name-keyed random entries (decoder_grad_ref.sample_index)
                        --, "max64:<name>" = max |f64| over the WHOLE tensor and "ref:<name>" = the reference's own figure
                        max |f32 - f64| / max |f64|, also over the whole tensor.
The reference layer runs in float64 on the CPU with module.double() and float64 as torch's default dtype for the run (its ConvGRU
creates the initial hidden state with torch.zeros(...) of the default dtype, :674); no op refuses float64.  The seed is advanced until the
float32 and the float64 run make the same discrete choices everywhere (decoder_grad_ref.discrete_steps: cameras, clamp and homo
gates, tap cells, the BEV floors, the refinement's clamps), each evaluated from its own precision's norm1 output and boxes.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import decoder_grad_ref as DR  # noqa: E402
import ref_loader  # noqa: E402

FIRST_SEED = 131


def run(ref, rmod, w, d, dtype):
    torch.set_default_dtype(dtype)       # (the reference's ConvGRU creates its initial state with torch.zeros(...) of the default dtype)
    rmod.to(dtype)
    rmod.load_state_dict({k: torch.from_numpy(v).to(dtype) for k, v in w.items()})
    rmod.zero_grad(set_to_none=True)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)  # noqa: E731
    leaves = {k: t(d[k]).requires_grad_() for k in ("query_bbox", "query_feat", "lss", "radar")}
    feats = [t(d[f"feat{i}"]).permute(0, 4, 1, 2, 3).contiguous().requires_grad_() for i in range(len(DR.HWS))]      # [S,C,N,H,W]
    metas = [dict(img_shape=[(DR.IMG_HW[0], DR.IMG_HW[1], 3)], time_diff=t(d["time_diff"]), lidar2img=t(d["lidar2img"]))]
    kept = {}
    hook = rmod.norm1.register_forward_hook(lambda m, i, o: kept.__setitem__("x1", o.detach()))
    feat, cls, pred = rmod(leaves["query_bbox"], leaves["query_feat"], feats, leaves["lss"], leaves["radar"], None, metas, layer=DR.LAYER)
    hook.remove()
    xy = sys.modules["models.bbox.utils"].theta_d2xy_coods(pred)
    ((feat * t(d["gout_feat"])).sum() + (cls * t(d["gout_cls"])).sum() + (xy * t(d["gout_xy"])).sum()).backward()
    g = {"p:" + k: p.grad.numpy().copy() for k, p in rmod.named_parameters()}
    g.update({k: v.grad.numpy().copy() for k, v in leaves.items()})
    g.update({f"feat{i}": f.grad.permute(0, 2, 3, 4, 1).contiguous().numpy() for i, f in enumerate(feats)})
    out = dict(out_feat=feat.detach().numpy(), out_cls=cls.detach().numpy(), out_pred=pred.detach().numpy(), out_xy=xy.detach().numpy())
    return g, out, DR.discrete_steps(w, d, kept["x1"], pred, dtype)


def main():
    torch.manual_seed(0)
    ref = ref_loader.load_reference()
    rmod = ref.racformer_transformer.RaCFormerTransformerDecoderLayer(**DR.LAYER_KW).eval()
    w = DR.make_weights({k: v.shape for k, v in rmod.state_dict().items()})
    seed = FIRST_SEED
    while True:
        d = DR.draw(seed)
        g32, out32, c32 = run(ref, rmod, w, d, torch.float32)
        g64, out64, c64 = run(ref, rmod, w, d, torch.float64)
        if DR.same_choices(c32, c64):
            break
        print(f"  seed {seed}: float32 and float64 differ in a discrete choice; next")
        seed += 1
    torch.set_default_dtype(torch.float32)
    gates = c64[1:5]
    print(f"  seed {seed}: clamped x/y {int((~gates[0]).sum())}/{int((~gates[1]).sum())}, homo <= eps {int((~gates[2]).sum())}, "
          f"no valid camera {int((~gates[3]).sum())}, BEV clamped {int((~c64[6]).sum())}/{int((~c64[9]).sum())}")
    assert int((~gates[0]).sum()) > 0 and int((~gates[3]).sum()) > 0 and int((~c64[6]).sum()) > 0
    gq = g32["query_bbox"]
    assert np.abs(gq[..., 8:]).max() == 0.0 and all(np.abs(gq[..., i]).max() > 0 for i in range(8))
    fx = dict(seed=np.array(seed), weight_seed=np.array(DR.WEIGHT_SEED))
    for k in ("query_bbox", "query_feat", "time_diff", "lidar2img", "gout_feat", "gout_cls", "gout_xy"):
        fx[k] = d[k]
    for k in ["lss", "radar"] + [f"feat{i}" for i in range(len(DR.HWS))]:
        assert np.array_equal(d[k].astype(np.float16).astype(np.float32), d[k])
        fx[k] = d[k].astype(np.float16)
    fx.update({k: v for k, v in out32.items()})
    fx.update({"out64_" + k[4:]: v for k, v in out64.items()})
    fx["weight_names"] = np.array(sorted(w))
    fx["weight_sums"] = np.array([w[k].astype(np.float64).sum() for k in sorted(w)])
    worst = ("", 0.0)
    for k in sorted(g64):
        m = float(np.abs(g64[k]).max())
        assert m > 0 and np.isfinite(g64[k]).all() and np.isfinite(g32[k]).all(), k
        figure = float(np.abs(g32[k].astype(np.float64) - g64[k]).max() / m)
        fx["g32:" + k], fx["g64:" + k] = DR.sampled(k, g32[k]), DR.sampled(k, g64[k])
        fx["max64:" + k], fx["ref:" + k] = np.array(m), np.array(figure)
        worst = max(worst, (k, figure), key=lambda x: x[1])
    print(f"  {len(g64)} gradient tensors; the reference's own worst float32 figure: {worst[1]:.2e} ({worst[0]})")
    figs = sorted(((float(fx[k]), k[4:]) for k in fx if k.startswith("ref:")), reverse=True)
    print("  largest figures:", ", ".join(f"{n} {v:.1e}" for v, n in figs[:6]), "; median %.1e" % figs[len(figs) // 2][0])
    # two files, each below the repository's 1 MiB limit for a committed file: the inputs and outputs, the gradients
    parts = {"decoder_grad_small.npz": {k: v for k, v in fx.items() if ":" not in k},
             "decoder_grad_small.1.npz": {k: v for k, v in fx.items() if ":" in k}}
    for name, part in parts.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **part)
        assert os.path.getsize(path) < 1024 * 1024, (name, os.path.getsize(path))
        print(f"  wrote {name}: {os.path.getsize(path) / 1024:.1f} KiB; {len(part)} keys")

if __name__ == "__main__":
    main()
