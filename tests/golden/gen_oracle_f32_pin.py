"""Writes tests/golden/oracle_f32_pin.npz: the float32 outputs and autograd gradients of the oracle's pure-torch gathers
(oracle/restate.py ``msmv_gather_torch`` / ``msda_torch``) on the committed golden inputs.

The committed file was written by the oracle as it stood before the gathers learned to follow their operands' dtype,
to round the view half away from zero and to form coordinates in float32 on request.  tests/test_backward_f64_cpu.py
asserts that the float32 results are still bit-identical to it.

    python tests/golden/gen_oracle_f32_pin.py [--restate path/to/restate.py]
"""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def load_restate(path):
    if path is None:
        sys.path.insert(0, ROOT)
        from oracle import restate
        return restate
    spec = importlib.util.spec_from_file_location("restate_pin", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def pinned_outputs(R, golden_dir=HERE):
    """name -> float32 array; every output the pin covers (shared with the test that checks it)."""
    t = lambda a: torch.from_numpy(np.asarray(a)).clone()
    res = {}
    g = np.load(os.path.join(golden_dir, "msmv_small.npz"))
    for tag, L in (("c45", 2), ("c2345", 4), ("c23456", 5)):
        feats = [t(g[f"{tag}_feat{i}"]) for i in range(L)]
        res[f"msmv_{tag}_out"] = R.msmv_gather_torch(feats, t(g[f"{tag}_loc"]), t(g[f"{tag}_w"]))
    m = np.load(os.path.join(golden_dir, "msda_small.npz"))
    res["msda_out"] = R.msda_torch(t(m["value"]), m["shapes"].tolist(), [0], t(m["loc"]), t(m["attn"]))
    sh2 = m["shapes2"].tolist()
    res["msda_out2"] = R.msda_torch(t(m["value2"]), sh2, [0, sh2[0][0] * sh2[0][1]], t(m["loc2"]), t(m["attn2"]))
    b = np.load(os.path.join(golden_dir, "backward_small.npz"))
    feats = [t(b[f"feat{i}"]).requires_grad_() for i in range(4)]
    loc, w = t(b["loc"]).requires_grad_(), t(b["w"]).requires_grad_()
    out = R.msmv_gather_torch(feats, loc, w)
    (out * t(b["gout"])).sum().backward()
    res["bwd_msmv_out"], res["bwd_msmv_gloc"], res["bwd_msmv_gw"] = out, loc.grad, w.grad
    for i in range(4):
        res[f"bwd_msmv_gfeat{i}"] = feats[i].grad
    v, ml, a = (t(b[k]).requires_grad_() for k in ("value", "mloc", "attn"))
    out = R.msda_torch(v, b["mshape"].tolist(), [0], ml, a)
    (out * t(b["mgout"])).sum().backward()
    res["bwd_msda_out"], res["bwd_msda_gvalue"], res["bwd_msda_gloc"], res["bwd_msda_gattn"] = out, v.grad, ml.grad, a.grad
    return {k: v.detach().numpy() for k, v in res.items()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--restate", default=None, help="oracle module to evaluate (default: this tree's oracle/restate.py)")
    ap.add_argument("--out", default=os.path.join(HERE, "oracle_f32_pin.npz"))
    args = ap.parse_args()
    torch.set_num_threads(1)
    outs = pinned_outputs(load_restate(args.restate))
    assert all(v.dtype == np.float32 for v in outs.values())
    np.savez_compressed(args.out, **outs)
    print(f"wrote {args.out}: {len(outs)} arrays")
