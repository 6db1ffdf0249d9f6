#!/usr/bin/env python3
"""Golden gradients of ScaleAdaptiveSelfAttention: runs the REFERENCE's own module (racformer_transformer.py:282-335, over
mmcv's MultiheadAttention with a float attn_mask) on CPU in eval mode (attention dropout off), backpropagates
sum(out * gout) for a seeded gout, and writes a data-only fixture next to this script.  Run in the build container only
(needs the reference tree, see ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_sasa_grad.py

  sasa_grad_small.npz   E = 128, 4 heads (head dim 32: the fused path), B = 2, Q = 37 (ragged against the 16-row tiles).
                        Inputs: query_bbox [B,Q,10], query_feat [B,Q,E], gout [B,Q,E], the module's weights under their
                        state_dict keys prefixed "w:".  Outputs: out, and under "g:" + the same keys the gradients of every
                        weight, and g:query_feat.  gen_tau is set so that head 0 has tau = 0 exactly (zero row, zero bias),
                        head 2 a negative tau and head 3 a large one (rows almost one-hot); some boxes share their centre
                        with another box (r = 0 off the diagonal).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_loader  # noqa: E402
from racformer_amd import synthetic as syn  # noqa: E402


def main():
    torch.manual_seed(0)
    ref = ref_loader.load_reference()
    rng = np.random.default_rng(53)
    B, Q, E, H = 2, 37, 128, 4
    mod = ref.racformer_transformer.ScaleAdaptiveSelfAttention(embed_dims=E, num_heads=H, dropout=0.1,
                                                               pc_range=syn.PC_RANGE).eval()
    sd = mod.state_dict()
    w = {}
    for k, v in sd.items():
        w[k] = (rng.standard_normal(tuple(v.shape), dtype=np.float32) * np.float32(1.5 / np.sqrt(E))).astype(np.float32)
    w["gen_tau.weight"] *= np.float32(0.2)
    w["gen_tau.weight"][0] = 0.0
    w["gen_tau.bias"][:] = np.array([0.0, 0.8, -0.3, 40.0], np.float32)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    qb = rng.random((B, Q, 10), dtype=np.float32)
    qb[:, 5] = qb[:, 2]                    # coincident centres (the same box twice)
    qb[1, 20:23] = qb[1, 7]
    qb[0, 30, 1] = 0.0                     # radius 0: the centre of the polar grid
    qf = rng.standard_normal((B, Q, E), dtype=np.float32)
    gout = rng.standard_normal((B, Q, E), dtype=np.float32)
    tqf = torch.from_numpy(qf).requires_grad_()
    tqb = torch.from_numpy(qb).requires_grad_()
    out = mod(tqb, tqf, None)
    (out * torch.from_numpy(gout)).sum().backward()
    assert tqb.grad is None or float(tqb.grad.abs().max()) == 0.0
    d = dict(query_bbox=qb, query_feat=qf, gout=gout, out=out.detach().numpy(), num_heads=np.array(H),
             **{"g:query_feat": tqf.grad.numpy()})
    for k, p in mod.named_parameters():
        d["w:" + k] = w[k]
        d["g:" + k] = p.grad.numpy()
    path = os.path.join(HERE, "sasa_grad_small.npz")
    np.savez_compressed(path, **d)
    print(f"  wrote sasa_grad_small.npz: {os.path.getsize(path) / 1024:.1f} KiB; keys {sorted(d)}")


if __name__ == "__main__":
    main()
