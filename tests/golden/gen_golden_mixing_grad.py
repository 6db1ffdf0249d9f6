#!/usr/bin/env python3
"""Golden gradients of AdaptiveMixing: runs the REFERENCE's own module (racformer_transformer.py:549-616) on CPU in eval
mode (inner_forward, no checkpointing), backpropagates sum(out * gout) for a seeded gout, and writes a data-only fixture next
to this script.  Run in the build container only (needs the reference tree, see ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_mixing_grad.py

  mixing_grad_small.npz   in_dim 128, G = 2 (64 channels per group: the fused path), P = 13 in points (odd: unaligned S rows),
                          128 out points, query_dim 4, B = 1, Q = 5.  Inputs: x [B,Q,G,P,64], query [B,Q,4], gout [B,Q,4], the
                          module's weights under their state_dict keys prefixed "w:" (f16-exact values, stored as float16).
                          Outputs: out, and under "g:" + the same keys the gradients of every weight, g:x and g:query.
  Every pre-activation (both LayerNorm outputs, before the ReLUs) is at least 2^-12 from zero, so a float32 kernel and the
  float64 restatement see the reference's ReLU masks.  A random draw cannot give that over ~90 000 pre-activations, so the
  signs are laid out: x[p] and the columns of M carry signs (sign_p * sign_d), S rows a sign of their own, each set far from
  zero by the generator's bias, which leaves A = x M and B = S Y in two well separated clusters on either side of their means.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_loader  # noqa: E402

MARGIN = 2.0 ** -12


def f16(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def main():
    torch.manual_seed(0)
    ref = ref_loader.load_reference()
    rng = np.random.default_rng(71)
    B, Q, G, P, C, OUT, QD = 1, 5, 2, 13, 64, 128, 4
    mod = ref.racformer_transformer.AdaptiveMixing(in_dim=G * C, in_points=P, n_groups=G, query_dim=QD, out_points=OUT).eval()
    tot = C * C + OUT * P
    # generator: small weights, a bias that fixes every generated value's sign and keeps it away from zero
    sign_d = np.where(rng.random(C) < 0.5, -1.0, 1.0)
    sign_o = np.where(rng.random(OUT) < 0.5, -1.0, 1.0)
    bias = np.empty((G, tot), np.float32)
    for g in range(G):
        bias[g, :C * C] = (sign_d[None, :] * rng.uniform(0.5, 1.5, (C, C))).reshape(-1)
        bias[g, C * C:] = (sign_o[:, None] * rng.uniform(0.5, 1.5, (OUT, P))).reshape(-1)
    w = {"parameter_generator.weight": f16(rng.standard_normal((G * tot, QD)) * 0.05),
         "parameter_generator.bias": f16(bias.reshape(-1)),
         "out_proj.weight": f16(rng.standard_normal((QD, G * OUT * C)) / np.sqrt(G * OUT * C)),
         "out_proj.bias": f16(rng.standard_normal(QD) * 0.1)}
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    sign_p = np.where(rng.random(P) < 0.5, -1.0, 1.0)
    sign_p[:2] = [1.0, -1.0]
    x = f16(sign_p[None, None, None, :, None] * rng.uniform(0.25, 1.5, (B, Q, G, P, C)))
    query = f16(rng.standard_normal((B, Q, QD)))
    gout = rng.standard_normal((B, Q, QD)).astype(np.float32)

    # margins of the pre-activations, in float64
    with torch.no_grad():
        prm = torch.from_numpy(query).double() @ torch.from_numpy(w["parameter_generator.weight"]).double().t() \
            + torch.from_numpy(w["parameter_generator.bias"]).double()
        prm = prm.reshape(B * Q, G, tot)
        M = prm[..., :C * C].reshape(B * Q, G, C, C)
        S = prm[..., C * C:].reshape(B * Q, G, OUT, P)
        worst = float("inf")
        a = torch.from_numpy(x).double().reshape(B * Q, G, P, C) @ M
        for t_ in (a, None):
            if t_ is None:
                t_ = S @ torch.relu(h)
            h = torch.nn.functional.layer_norm(t_, t_.shape[-2:])
            worst = min(worst, float(h.abs().min()))
    assert worst >= MARGIN, f"a pre-activation lies {worst:.3g} from zero"

    tx = torch.from_numpy(x).requires_grad_()
    tq = torch.from_numpy(query).requires_grad_()
    out = mod(tx, tq)
    (out * torch.from_numpy(gout)).sum().backward()
    d = dict(x=x, query=query, gout=gout, out=out.detach().numpy(), in_points=np.array(P), n_groups=np.array(G),
             **{"g:x": tx.grad.numpy(), "g:query": tq.grad.numpy()})
    for k, p in mod.named_parameters():
        d["w:" + k] = w[k].astype(np.float16)
        d["g:" + k] = p.grad.numpy()
    path = os.path.join(HERE, "mixing_grad_small.npz")
    np.savez_compressed(path, **d)
    print(f"  wrote mixing_grad_small.npz: {os.path.getsize(path) / 1024:.1f} KiB; least |pre-activation| {worst:.3g}; "
          f"keys {sorted(d)}")


if __name__ == "__main__":
    main()
