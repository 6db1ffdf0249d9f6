"""msmv_sampling_v2 (rac_msmv_v2_fwd / rac_msmv_v2_bwd) on the MI355X: the reference's goldens in both feature layouts, a
random sweep against the oracle through the one-hot identity (v2 == the weighted operator with one-hot argmax weights),
bf16 features, the f8 full size, the backward's properties, graph capture and sampling_4d(aggregate=False)."""
import os

import numpy as np
import pytest
import torch

from oracle import restate as R
from racformer_amd import _lib, synthetic as syn
from racformer_amd import transformer as T
from racformer_amd.msmv import msmv_backward, msmv_sampling_v2, msmv_v2_backward, msmv_v2_forward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def t(a):
    return torch.from_numpy(np.asarray(a))


def maxerr(a, b):
    return (a.detach().cpu().double() - torch.as_tensor(b).double()).abs().max().item()


def onehot_argmax(w):
    return torch.nn.functional.one_hot(torch.argmax(w, dim=-1), w.shape[-1]).to(torch.float32)


def _golden(golden_dir, L):
    g = np.load(os.path.join(golden_dir, "msmv_v2_small.npz"))
    k = f"l{L}_"
    return g, k, [t(g[f"{k}feat{i}"]) for i in range(L)]


@pytest.mark.parametrize("L", [2, 4, 5])
@pytest.mark.parametrize("channels_first", [False, True])
def test_v2_golden_forward_backward(golden_dir, L, channels_first):
    g, k, feats = _golden(golden_dir, L)
    if channels_first:
        feats = [f.permute(0, 4, 1, 2, 3).contiguous() for f in feats]
    gf = [f.to(DEV).requires_grad_() for f in feats]
    loc = t(g[k + "loc"]).to(DEV).requires_grad_()
    w = t(g[k + "w"]).to(DEV).requires_grad_()
    out = msmv_sampling_v2(gf, loc, w, channels_first=channels_first)
    assert out.shape == g[k + "out"].shape
    assert maxerr(out, g[k + "out"]) < 2e-5            # the reference is trilinear in the view axis
    (out * t(g[k + "gout"]).to(DEV)).sum().backward()
    for i in range(L):
        got = gf[i].grad.permute(0, 2, 3, 4, 1) if channels_first else gf[i].grad
        assert maxerr(got, g[f"{k}gfeat{i}"]) < 2e-5, i
    assert maxerr(loc.grad[..., :2], t(g[k + "gloc"])[..., :2]) < 2e-4
    assert loc.grad[..., 2].abs().max().item() == 0.0   # view component: exactly 0, as rac_msmv_bwd
    assert w.grad is None                                 # argmax cuts the graph


def _rand_case(seed, S, N, Q, P, C, hws):
    rng = np.random.default_rng(seed)
    L = len(hws)
    feats = [t(rng.standard_normal((S, N, h, w, C), dtype=np.float32)) for h, w in hws]
    loc = rng.random((S, Q, P, 3), dtype=np.float32) * 1.1 - 0.05
    loc[..., 2] = rng.integers(0, N, size=(S, Q, P)).astype(np.float32) / np.float32(max(N - 1, 1))
    loc[0, 0, 0, :2] = (0.0, 0.0)
    loc[0, 0, P - 1, :2] = (1.0, 1.0)
    loc[0, Q - 1, 0, :2] = (-1e5, 0.5)
    loc[S - 1, Q - 1, P - 1, :2] = (1.0 + 1e-3, -1e-3)
    w = rng.random((S, Q, P, L), dtype=np.float32)
    w[:, ::2, ::3] = 0.25                                             # tie rows: level 0
    w[:, 1::3, 1::2, L - 1] = w[:, 1::3, 1::2].max(-1)                # tie between the maximum and the last level
    return feats, t(loc), t(w)


@pytest.mark.parametrize("S,N,Q,P,L", [(3, 2, 5, 12, 4), (9, 6, 7, 3, 4), (2, 3, 4, 1, 2), (8, 1, 9, 13, 5),
                                       (1, 6, 1, 128, 4), (2, 6, 3, 128, 2)])
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("C", [8, 64])
def test_v2_random_sweep(S, N, Q, P, L, layout, C):
    """ragged Q, P = 1 and at the 128 limit, one view, both output layouts, the C = 64 fast path and the generic one"""
    hws = [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)][:L]
    feats, loc, w = _rand_case(S * 100 + P + C, S, N, Q, P, C, hws)
    ref = R.msmv_gather(feats, loc, onehot_argmax(w))                  # [S,Q,C,P]
    T_, G_ = (1, S) if layout else (1, 1)
    for channels_first in (False, True):
        gf = [(f.permute(0, 4, 1, 2, 3) if channels_first else f).contiguous().to(DEV) for f in feats]
        out = msmv_v2_forward(gf, loc.to(DEV), w.to(DEV), out_layout=layout, num_frames=T_, num_groups=G_,
                              channels_first=channels_first)
        if layout:   # [B=1,Q,G=S,T*P,C] -> [S,Q,C,P]
            out = out.reshape(1, Q, S, 1, P, C).permute(0, 3, 2, 1, 5, 4).reshape(S, Q, C, P)
        assert maxerr(out, ref) < 1e-5, channels_first


def test_v2_bf16_features():
    hws = [(12, 20), (6, 10), (3, 5), (2, 3)]
    for C in (64, 8):
        feats, loc, w = _rand_case(5 + C, 4, 3, 6, 12, C, hws)
        feats = [f.to(torch.bfloat16).float() for f in feats]           # the oracle sees the rounded values
        ref = R.msmv_gather(feats, loc, onehot_argmax(w))
        out = msmv_v2_forward([f.to(DEV).to(torch.bfloat16) for f in feats], loc.to(DEV), w.to(DEV))
        assert maxerr(out, ref) < 1e-5, C
    with pytest.raises(RuntimeError, match="float32"):
        msmv_v2_forward([f.to(DEV).to(torch.bfloat16).permute(0, 4, 1, 2, 3).contiguous() for f in feats], loc.to(DEV),
                        w.to(DEV), channels_first=True)


def test_v2_errors_and_empty():
    hws = [(4, 6), (2, 3)]
    feats, loc, w = _rand_case(2, 2, 2, 3, 4, 64, hws)
    gf = [f.to(DEV) for f in feats]
    with pytest.raises(RuntimeError, match="contiguous"):
        msmv_sampling_v2(gf, loc.to(DEV)[:, :, ::2], w.to(DEV)[:, :, ::2])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        msmv_sampling_v2(gf, loc, w.to(DEV))
    with pytest.raises(RuntimeError, match="num_point exceed limits"):
        msmv_sampling_v2(gf, torch.zeros(2, 3, 129, 3, device=DEV), torch.zeros(2, 3, 129, 2, device=DEV))
    with pytest.raises(RuntimeError, match="scale_weights"):
        msmv_sampling_v2(gf, loc.to(DEV), torch.zeros(2, 3, 4, 3, device=DEV))
    out = msmv_sampling_v2(gf, torch.zeros(2, 0, 4, 3, device=DEV), torch.zeros(2, 0, 4, 2, device=DEV))
    assert out.shape == (2, 0, 64, 4)


def _f8_case():
    cfg = syn.F8
    S, N, Q, P, C = 32, 6, 900, 12, 64
    rng = np.random.default_rng(0)
    feats = [t(syn.smooth_noise(70 + i, (S, N), h, w * C).reshape(S, N, h, w, C)) for i, (h, w) in enumerate(cfg.fpn_hw)]
    loc = rng.random((S, Q, P, 3), dtype=np.float32) * 1.1 - 0.05
    loc[..., 2] = rng.integers(0, N, size=(S, Q, P)).astype(np.float32) / np.float32(N - 1)
    w = rng.standard_normal((S, Q, P, 4), dtype=np.float32)
    w = np.exp(w) / np.exp(w).sum(-1, keepdims=True)
    return feats, t(loc), t(w.astype(np.float32))


def test_v2_f8_full_size():
    """f8 shapes (S=32, N=6, Q=900, P=12, C=64, 4 levels) against the C oracle with one-hot weights; the backward against
    rac_msmv_bwd with the same one-hot weights (the same sums: the other levels contribute exact zeros)"""
    feats, loc, w = _f8_case()
    S, Q, P, C = 32, 900, 12, 64
    oh = onehot_argmax(w)
    ref = R.msmv_gather(feats, loc, oh)
    gf, gl, gw = [f.to(DEV) for f in feats], loc.to(DEV), w.to(DEV)
    out0 = msmv_v2_forward(gf, gl, gw)
    assert maxerr(out0, ref) < 1e-5
    out1 = msmv_v2_forward(gf, gl, gw, out_layout=_lib.OUT_BQGTPC, num_frames=8, num_groups=4)
    assert torch.equal(out1, out0.reshape(1, 8, 4, Q, C, P).permute(0, 3, 2, 1, 5, 4).flatten(3, 4))
    far = gl.clone()
    far[..., 0] = 5.0
    assert msmv_v2_forward(gf, far, gw).abs().max().item() == 0.0
    gout = torch.from_numpy(np.random.default_rng(1).standard_normal((S, Q, C, P), dtype=np.float32)).to(DEV)
    gfe, gloc = msmv_v2_backward(gout, gf, gl, gw)
    rfe, rloc, _ = msmv_backward(gout, gf, gl, oh.to(DEV))
    for a, b in zip(gfe, rfe):   # (float atomics: the order of the adds differs)
        assert (a - b).abs().max().item() <= 1e-5 * max(1.0, b.abs().max().item())
    assert (gloc - rloc).abs().max().item() <= 1e-4 * max(1.0, rloc.abs().max().item())
    assert gloc[..., 2].abs().max().item() == 0.0
    # deterministic per-point gradients: a second run gives the same bits
    _, gloc2 = msmv_v2_backward(gout, gf, gl, gw)
    assert torch.equal(gloc, gloc2)


def test_v2_backward_deterministic_generic_path():
    feats, loc, w = _rand_case(11, 3, 3, 7, 9, 8, [(12, 20), (6, 10), (3, 5), (2, 3)])
    for channels_first in (False, True):
        gf = [(f.permute(0, 4, 1, 2, 3) if channels_first else f).contiguous().to(DEV) for f in feats]
        gout = torch.randn(3, 7, 8, 9, generator=torch.Generator().manual_seed(2)).to(DEV)
        _, a = msmv_v2_backward(gout, gf, loc.to(DEV), w.to(DEV), channels_first=channels_first)
        _, b = msmv_v2_backward(gout, gf, loc.to(DEV), w.to(DEV), channels_first=channels_first)
        assert torch.equal(a, b)
        assert a[..., 2].abs().max().item() == 0.0


def test_v2_graph_capture_replay():
    """no host sync and no allocation inside the launch: a captured forward replays to the eager bits"""
    feats, loc, w = _rand_case(4, 4, 6, 33, 12, 64, [(12, 20), (6, 10), (3, 5), (2, 3)])
    gf, gl, gw = [f.to(DEV) for f in feats], loc.to(DEV), w.to(DEV)
    eager = msmv_v2_forward(gf, gl, gw)
    out = torch.empty_like(eager)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        msmv_v2_forward(gf, gl, gw, out=out)                          # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    out.zero_()
    with torch.cuda.graph(graph):
        msmv_v2_forward(gf, gl, gw, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_sampling_4d_hard_level_golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "sampling4d_v2_small.npz"))
    H, W = (int(x) for x in g["image_hw"])
    feats = [t(g[f"feat{i}"]).to(DEV) for i in range(4)]
    final, homo, i_view = T.sampling_4d(t(g["pts"]).to(DEV), feats, t(g["scale_weights"]).to(DEV), t(g["lidar2img"]).to(DEV),
                                        H, W, aggregate=False)
    assert final.shape == g["final"].shape and homo.shape == g["homo"].shape and i_view.shape == g["i_view"].shape
    assert i_view.dtype == torch.int64 and homo.dtype == torch.float32
    assert torch.equal(i_view.cpu(), t(g["i_view"]))
    assert torch.allclose(homo.cpu(), t(g["homo"]), rtol=1e-5, atol=1e-4)
    assert maxerr(final, g["final"]) < 2e-5
