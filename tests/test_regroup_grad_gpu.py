"""Backward of the pyramid regroup on the MI355X (rac_regroup_multi_bwd / rac_regroup_bwd through regroup_pyramid's autograd
route): a pure permutation, so the gradients must be BITWISE the torch restatement
``grad.view(B,T,G,N,H,W,C).permute(0,1,3,2,6,4,5)`` of a seeded random gradient.  Shapes chosen for the tile edges (64 x 64 tiles):
a level that is a single partial pixel tile, one with H*W < 64, a partial channel tile, sizes that are no multiple of 4 (the scalar
per-level kernel), and a pyramid of which only some levels require grad."""
import pytest
import torch

from racformer_amd import transformer as T

pytestmark = pytest.mark.gpu
B, TF, N, G = 2, 2, 3, 4
PYRAMID = [(8, 22), (4, 11), (2, 6), (1, 4)]
CASES = {"a_c64": (64, PYRAMID, None), "b_c20_partial_channel_tile": (20, PYRAMID, None), "c_scalar_path": (6, [(3, 5)], None),
         "d_levels_0_and_2_only": (64, PYRAMID, (0, 2))}


def make(C, levels, seed):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(B, TF * N, G * C, h, w, generator=g).cuda() for h, w in levels]
    gouts = [torch.randn(B * TF * G, N, h, w, C, generator=g).cuda() for h, w in levels]
    return feats, gouts


def restated(gout, C):
    H, W = gout.shape[2:4]
    return gout.view(B, TF, G, N, H, W, C).permute(0, 1, 3, 2, 6, 4, 5).reshape(B, TF * N, G * C, H, W).contiguous()


def run(C, levels, live, seed=5):
    feats, gouts = make(C, levels, seed)
    with torch.no_grad():
        plain = T.regroup_pyramid(list(feats), N, G)
    for l, f in enumerate(feats):
        f.requires_grad_(live is None or l in live)
    outs = T.regroup_pyramid(list(feats), N, G)
    torch.autograd.backward(outs, gouts)
    torch.cuda.synchronize()
    return feats, gouts, plain, outs


@pytest.mark.parametrize("name", list(CASES))
def test_gradient_is_bitwise_the_permutation(name):
    C, levels, live = CASES[name]
    feats, gouts, plain, outs = run(C, levels, live)
    for l, (f, go, p, o) in enumerate(zip(feats, gouts, plain, outs)):
        assert o.grad_fn is not None and torch.equal(o, p), f"level {l}: the output under grad is not the no_grad output"
        if live is not None and l not in live:
            assert f.grad is None
            continue
        assert f.grad.shape == f.shape and f.grad.dtype == torch.float32
        assert torch.equal(f.grad, restated(go, C)), f"level {l}"
    again = run(C, levels, live)[0]
    assert all((a.grad is None and b.grad is None) or torch.equal(a.grad, b.grad) for a, b in zip(feats, again))


def test_forward_under_grad_is_the_reference_permutation():
    """(the regroup itself, restated: what the gradient above is the transpose of)"""
    feats, _, plain, _ = run(64, PYRAMID, None)
    for f, p in zip(feats, plain):
        H, W = f.shape[3:]
        want = f.detach().view(B, TF, N, G, 64, H, W).permute(0, 1, 3, 2, 5, 6, 4).reshape(B * TF * G, N, H, W, 64)
        assert torch.equal(p, want)


def test_half_precision_and_strided_producers_get_their_gradient():
    """the cast and the compaction in front of the kernel stay torch ops"""
    feats, gouts = make(64, PYRAMID[:2], 6)
    half = feats[0].half().requires_grad_()
    strided = feats[1].transpose(3, 4).contiguous().transpose(3, 4).requires_grad_()
    assert not strided.is_contiguous()
    outs = T.regroup_pyramid([half, strided], N, G)
    torch.autograd.backward(outs, gouts)
    assert half.grad.dtype == torch.float16 and torch.equal(half.grad, restated(gouts[0], 64).half())
    assert torch.equal(strided.grad, restated(gouts[1], 64))


def test_bf16_output_raises_at_backward_time():
    feats, gouts = make(64, PYRAMID[:2], 7)
    for f in feats:
        f.requires_grad_()
    outs = T.regroup_pyramid(list(feats), N, G, out_dtype=torch.bfloat16)
    assert outs[0].dtype == torch.bfloat16 and outs[0].grad_fn is not None
    with pytest.raises(RuntimeError, match="float32 features only"):
        torch.autograd.backward(outs, [g.bfloat16() for g in gouts])


def test_frozen_pyramid_takes_the_plain_launch():
    feats, _ = make(64, PYRAMID, 8)
    outs = T.regroup_pyramid(list(feats), N, G)
    assert all(o.grad_fn is None for o in outs)
