#!/usr/bin/env python3
"""Golden gradients of one decoder layer at B = 2: the REFERENCE's own RaCFormerTransformerDecoderLayer on the rig of
tests/decoder_grad_ref.py with two samples (two seeded draws of decoder_grad_ref.draw, concatenated along the batch), in float32 and
float64 on the CPU, exactly as gen_golden_decoder_grad.py runs it at B = 1 (whose run() and layout this script uses).  At B = 2 the
reference's BEV attention pairs frames and batches (models/bev_self_attention.py:162-218); the fixture holds what it computes.
Run in the build container only (needs the reference tree, see ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_decoder_grad_b2.py

  decoder_grad_small_b2.npz   data only, the keys of decoder_grad_small.npz + decoder_grad_small.1.npz in one file: the two seeds
                              (the inputs are a function of them and are not stored), the outputs in float32 and float64 and,
                              per gradient tensor, "g64:" (sampled as there), "max64:" and "ref:" (the float32 gradients are not
                              kept: the checks read the float64 ones and the figure).
The second seed is advanced until float32 and float64 make the same discrete choices in both samples
(decoder_grad_ref.discrete_steps, sample by sample: the pairing permutes which frame a keypoint reads, not the keypoints)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import decoder_grad_ref as DR  # noqa: E402
import gen_golden_decoder_grad as G1  # noqa: E402
import ref_loader  # noqa: E402

FIRST_SEEDS = (131, 140)


def draw_b2(seeds):
    ds = [DR.draw(s) for s in seeds]
    return {k: np.concatenate([d[k] for d in ds], axis=0) for k in ds[0]}


def run(ref, rmod, w, d, dtype):
    """G1.run with the discrete choices evaluated sample by sample"""
    real = DR.discrete_steps

    def per_sample(w_, d_, x1, pred, dtype_):
        res = []
        for b in range(2):
            db = {k: (v[b * (len(v) // 2):(b + 1) * (len(v) // 2)] if isinstance(v, np.ndarray) else v) for k, v in d_.items()}
            res += real(w_, db, x1[b:b + 1], pred[b:b + 1], dtype_)
        return res

    DR.discrete_steps = per_sample
    try:
        return G1.run(ref, rmod, w, d, dtype)
    finally:
        DR.discrete_steps = real


def main():
    torch.manual_seed(0)
    ref = ref_loader.load_reference()
    rmod = ref.racformer_transformer.RaCFormerTransformerDecoderLayer(**DR.LAYER_KW).eval()
    w = DR.make_weights({k: v.shape for k, v in rmod.state_dict().items()})
    seeds = list(FIRST_SEEDS)
    while True:
        d = draw_b2(seeds)
        g32, out32, c32 = run(ref, rmod, w, d, torch.float32)
        g64, out64, c64 = run(ref, rmod, w, d, torch.float64)
        if DR.same_choices(c32, c64):
            break
        print(f"  seeds {seeds}: float32 and float64 differ in a discrete choice; next")
        seeds[1] += 1
    torch.set_default_dtype(torch.float32)
    gq = g32["query_bbox"]
    assert gq.shape[0] == 2 and np.abs(gq[..., 8:]).max() == 0.0 and all(np.abs(gq[..., i]).max() > 0 for i in range(8))
    fx = dict(seeds=np.array(seeds), weight_seed=np.array(DR.WEIGHT_SEED))
    fx.update({k: v for k, v in out32.items()})
    fx.update({"out64_" + k[4:]: v for k, v in out64.items()})
    worst = ("", 0.0)
    for k in sorted(g64):
        m = float(np.abs(g64[k]).max())
        assert m > 0 and np.isfinite(g64[k]).all() and np.isfinite(g32[k]).all(), k
        figure = float(np.abs(g32[k].astype(np.float64) - g64[k]).max() / m)
        fx["g64:" + k] = DR.sampled(k, g64[k])
        fx["max64:" + k], fx["ref:" + k] = np.array(m), np.array(figure)
        worst = max(worst, (k, figure), key=lambda x: x[1])
    print(f"  seeds {seeds}: {len(g64)} gradient tensors; the reference's own worst float32 figure: {worst[1]:.2e} ({worst[0]})")
    path = os.path.join(HERE, "decoder_grad_small_b2.npz")
    np.savez_compressed(path, **fx)
    assert os.path.getsize(path) < 1024 * 1024, os.path.getsize(path)
    print(f"  wrote decoder_grad_small_b2.npz: {os.path.getsize(path) / 1024:.1f} KiB; {len(fx)} keys")


if __name__ == "__main__":
    main()
