#!/usr/bin/env python3
"""Golden gradients of ScaleAdaptiveSelfAttention under a boolean attention mask: runs the REFERENCE's own module
(racformer_transformer.py:282-335, ``mask[:, :, pre_attn_mask] = -inf`` at :311-312) on CPU in eval mode (attention dropout
off), backpropagates sum(out * gout) for a seeded gout, and writes a data-only fixture next to this script.  Run in the build
container only (needs the reference tree, see ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_sasa_mask_grad.py

  sasa_mask_grad_small.npz  E = 128, 4 heads (head dim 32: the fused path), B = 2.  The mask is the query-denoising layout
                        (racformer_head.py:220-232) with 3 groups of 7 denoising queries in front of 20 matching queries:
                        Q = 41, ragged against the 16-row tiles and the 32-bit mask words.  Weights and boxes follow
                        gen_golden_sasa_grad.py: head 0 has tau = 0 exactly, head 2 a negative tau, head 3 a large one; some
                        boxes share their centre.  Inputs: query_bbox, query_feat, gout, attn_mask (bool [Q,Q], True: blocked),
                        the weights under "w:" + state_dict key.  Outputs: out, "g:" + key for every weight, g:query_feat, in
                        float32; the same from a float64 run of the same module under "out64" / "g64:" + key (every tensor of at most
                        4096 elements: the output, query_feat, the biases and gen_tau; computed in float64, stored as float32).
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


def dn_mask(groups, single, matching):
    """the loop of racformer_head.py:220-232, restated on index arithmetic"""
    pad, Q = groups * single, groups * single + matching
    idx = np.arange(Q)
    group = np.where(idx < pad, idx // single, -1)
    return (idx[None, :] < pad) & (group[:, None] != group[None, :])


def run(mod, qb, qf, gout, mask, dtype):
    mod = mod.to(dtype)
    mod.zero_grad(set_to_none=True)
    tqf = torch.from_numpy(qf).to(dtype).requires_grad_()
    tqb = torch.from_numpy(qb).to(dtype).requires_grad_()
    out = mod(tqb, tqf, torch.from_numpy(mask))
    (out * torch.from_numpy(gout).to(dtype)).sum().backward()
    assert tqb.grad is None or float(tqb.grad.abs().max()) == 0.0
    return out.detach().numpy(), tqf.grad.numpy(), {k: p.grad.numpy().copy() for k, p in mod.named_parameters()}


def main():
    torch.manual_seed(0)
    ref = ref_loader.load_reference()
    rng = np.random.default_rng(59)
    B, E, H = 2, 128, 4
    mask = dn_mask(3, 7, 20)
    Q = mask.shape[0]
    mod = ref.racformer_transformer.ScaleAdaptiveSelfAttention(embed_dims=E, num_heads=H, dropout=0.1,
                                                               pc_range=syn.PC_RANGE).eval()
    w = {}
    for k, v in mod.state_dict().items():
        w[k] = (rng.standard_normal(tuple(v.shape), dtype=np.float32) * np.float32(1.5 / np.sqrt(E))).astype(np.float32)
    w["gen_tau.weight"] *= np.float32(0.2)
    w["gen_tau.weight"][0] = 0.0
    w["gen_tau.bias"][:] = np.array([0.0, 0.8, -0.3, 40.0], np.float32)
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    qb = rng.random((B, Q, 10), dtype=np.float32)
    qb[:, 5] = qb[:, 2]                    # coincident centres inside a denoising group
    qb[1, 25:28] = qb[1, 8]                # matching queries on a denoising query's centre
    qb[0, 33, 1] = 0.0                     # radius 0: the centre of the polar grid
    qf = rng.standard_normal((B, Q, E), dtype=np.float32)
    gout = rng.standard_normal((B, Q, E), dtype=np.float32)
    out, gqf, gw = run(mod, qb, qf, gout, mask, torch.float32)
    d = dict(query_bbox=qb, query_feat=qf, gout=gout, attn_mask=mask, out=out, num_heads=np.array(H), **{"g:query_feat": gqf})
    for k in gw:
        d["w:" + k] = w[k]
        d["g:" + k] = gw[k]
    out64, gqf64, gw64 = run(mod, qb, qf, gout, mask, torch.float64)
    # (the two large matrices' float64 gradients are left out: they would double the fixture;
    # and what is kept is stored rounded to float32 -- 6e-8 of each value, far inside the 2e-5 the tests ask for)
    d.update(out64=out64.astype(np.float32), **{"g64:query_feat": gqf64.astype(np.float32)},
             **{"g64:" + k: v.astype(np.float32) for k, v in gw64.items() if v.size <= 4096})
    path = os.path.join(HERE, "sasa_mask_grad_small.npz")
    np.savez_compressed(path, **d)
    print(f"  wrote sasa_mask_grad_small.npz: {os.path.getsize(path) / 1024:.1f} KiB; keys {sorted(d)}")


if __name__ == "__main__":
    main()
