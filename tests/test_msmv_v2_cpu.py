"""msmv_sampling_v2 / sampling_4d(aggregate=False) without a GPU: the reference's goldens against the oracle through the
one-hot identity (v2 equals the weighted operator with one-hot argmax weights), the host logic of
sampling_4d(aggregate=False) with the HIP launcher replaced by that oracle, and the argument checks of the two C entry
points (they return before any HIP call)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import restate as R
from racformer_amd import _lib
from racformer_amd import transformer as T


def t(a):
    return torch.from_numpy(np.asarray(a))


def onehot_argmax(w):
    """the weights that make the weighted operator equal v2: one-hot of torch.argmax (ties first, NaN maximal)"""
    return torch.nn.functional.one_hot(torch.argmax(w, dim=-1), w.shape[-1]).to(torch.float32)


def test_import_surface():
    from racformer_amd.msmv import MSMVSamplingV2, msmv_sampling, msmv_sampling_v2  # noqa: F401  (sparsebev_sampling.py:5)
    assert callable(msmv_sampling_v2)


def test_argmax_rules_of_the_fixture():
    """the crafted rows pin torch.argmax's rules, which the kernel reproduces"""
    w = torch.tensor([[.3, .3, .1, .3], [.1, float("nan"), .5, float("nan")], [-float("inf")] * 4,
                      [.9, .1, .1, float("nan")]])
    assert torch.argmax(w, dim=-1).tolist() == [0, 1, 0, 3]


@pytest.mark.parametrize("L", [2, 4, 5])
def test_golden_vs_onehot_oracle(golden_dir, L):
    g = np.load(os.path.join(golden_dir, "msmv_v2_small.npz"))
    k = f"l{L}_"
    w = t(g[k + "w"])
    assert torch.isnan(w).any() and torch.isinf(w).any()
    feats = [t(g[f"{k}feat{i}"]).clone().requires_grad_() for i in range(L)]
    loc = t(g[k + "loc"]).clone().requires_grad_()
    out = R.msmv_gather_torch(feats, loc, onehot_argmax(w))
    assert out.shape == g[k + "out"].shape
    assert (out.detach() - t(g[k + "out"])).abs().max().item() < 2e-5   # the reference is trilinear in the view axis
    (out * t(g[k + "gout"])).sum().backward()
    for i in range(L):
        assert (feats[i].grad - t(g[f"{k}gfeat{i}"])).abs().max().item() < 2e-5, i
    assert (loc.grad[..., :2] - t(g[k + "gloc"])[..., :2]).abs().max().item() < 2e-4
    # the fixture exercises levels beyond 0 and points with no gradient at all (outside every map)
    assert len(set(torch.argmax(w, -1).reshape(-1).tolist())) == L


def _oracle_v2(feats, loc, w, out_layout=0, num_frames=1, num_groups=1, channels_first=False, out=None):
    assert not channels_first
    o = R.msmv_gather(list(feats), loc, onehot_argmax(w))       # [S,Q,C,P]
    if out_layout == 0:
        return o
    S, Q, C, P = o.shape
    B = S // (num_frames * num_groups)
    return o.reshape(B, num_frames, num_groups, Q, C, P).permute(0, 3, 2, 1, 5, 4).flatten(3, 4).contiguous()


def test_sampling_4d_hard_level_host_logic(golden_dir, monkeypatch):
    monkeypatch.setattr(T, "msmv_v2_forward", _oracle_v2)
    g = np.load(os.path.join(golden_dir, "sampling4d_v2_small.npz"))
    H, W = (int(x) for x in g["image_hw"])
    feats = [t(g[f"feat{i}"]) for i in range(4)]
    final, homo, i_view = T.sampling_4d(t(g["pts"]), feats, t(g["scale_weights"]), t(g["lidar2img"]), H, W, aggregate=False)
    for name, got in (("final", final), ("homo", homo), ("i_view", i_view)):
        assert tuple(got.shape) == g[name].shape, name
        assert str(got.dtype).replace("torch.", "") == str(g[name].dtype), name
    assert torch.equal(i_view, t(g["i_view"]))
    assert torch.allclose(homo, t(g["homo"]), rtol=1e-5, atol=1e-4)
    assert (final - t(g["final"])).abs().max().item() < 2e-5
    # the fixture holds points visible in no camera: they sample view 0
    B, Q, Tf, G, P, _ = g["pts"].shape
    _, _, seen = R.project_select(t(g["pts"]).reshape(B, Q, Tf, G * P, 3), t(g["lidar2img"]), H, W)
    assert not bool(seen[:, 0].all())
    # the aggregate path is unchanged: still one tensor
    monkeypatch.setattr(T, "msmv_forward", lambda f, loc, w, **kw: _oracle_v2(f, loc, w, **kw))
    assert isinstance(T.sampling_4d(t(g["pts"]), feats, t(g["scale_weights"]), t(g["lidar2img"]), H, W), torch.Tensor)


def test_sampling_4d_hard_level_imposed_views(golden_dir, monkeypatch):
    """i_view reports the camera actually sampled: the imposed one under view_in"""
    monkeypatch.setattr(T, "msmv_v2_forward", _oracle_v2)
    g = np.load(os.path.join(golden_dir, "sampling4d_v2_small.npz"))
    H, W = (int(x) for x in g["image_hw"])
    B, Q, Tf, G, P, _ = g["pts"].shape
    N = g["lidar2img"].shape[1] // Tf
    forced = torch.from_numpy(np.random.default_rng(3).integers(0, N, size=(B * Tf * G, Q, P)).astype(np.uint8))
    _, _, i_view = T.sampling_4d(t(g["pts"]), [t(g[f"feat{i}"]) for i in range(4)], t(g["scale_weights"]), t(g["lidar2img"]),
                                 H, W, aggregate=False, view_in=forced)
    want = forced.long().view(B, Tf, G, Q, P)[:, 0].permute(0, 2, 1, 3).reshape(B, Q, G * P, 1)
    assert torch.equal(i_view, want)


def _lib_or_skip():
    try:
        return _lib.lib()
    except RuntimeError as e:
        pytest.fail(str(e))


def test_capi_argument_errors():
    lib = _lib_or_skip()
    dummy = ctypes.c_void_p(16)                     # never dereferenced: every call below fails its checks first
    feats = (ctypes.c_void_p * 2)(16, 16)
    hw = (ctypes.c_int32 * 4)(4, 6, 2, 3)
    null_feats = (ctypes.c_void_p * 2)(16, None)

    def fwd(feats=feats, hw=hw, L=2, loc=dummy, w=dummy, out=dummy, S=2, N=3, Q=4, P=5, C=64, dtype=_lib.RAC_F32,
            feat_layout=_lib.FEAT_CL, out_layout=_lib.OUT_SQCP, T_=1, G=1):
        return lib.rac_msmv_v2_fwd(feats, hw, L, loc, w, out, S, N, Q, P, C, dtype, feat_layout, out_layout, T_, G, None)

    def last():
        return lib.rac_last_error().decode()

    assert fwd(L=0) == -1 and "L=0" in last()
    assert fwd(L=9) == -1
    assert fwd(P=129) == -1 and "num_point exceed limits" in last()
    assert fwd(N=0) == -1
    assert fwd(dtype=7) == -1
    assert fwd(feat_layout=2) == -1 and "feature layout" in last()
    assert fwd(feat_layout=_lib.FEAT_CF, dtype=_lib.RAC_BF16) == -1 and "float32" in last()
    assert fwd(out_layout=5) == -1
    assert fwd(out_layout=_lib.OUT_BQGTPC, T_=3, G=1) == -1 and "multiple" in last()
    assert fwd(feats=None) == -1 and "null" in last()
    assert fwd(feats=null_feats) == -1 and "level 1" in last()
    assert fwd(loc=None) == -1
    assert fwd(out=None) == -1
    assert fwd(hw=(ctypes.c_int32 * 4)(4, 6, 0, 3)) == -1 and "empty map" in last()
    assert fwd(Q=0, out=None, loc=None) == 0        # empty output: nothing to check or launch

    gfeats = (ctypes.c_void_p * 2)(32, 32)

    def bwd(gout=dummy, feats=feats, hw=hw, L=2, loc=dummy, w=dummy, gfeats=gfeats, gloc=dummy, S=2, N=3, Q=4, P=5, C=64,
            feat_layout=_lib.FEAT_CL):
        return lib.rac_msmv_v2_bwd(gout, feats, hw, L, loc, w, gfeats, gloc, S, N, Q, P, C, feat_layout, None)

    assert bwd(L=0) == -1
    assert bwd(P=200) == -1 and "num_point exceed limits" in last()
    assert bwd(feat_layout=-1) == -1
    assert bwd(gout=None) == -1
    assert bwd(gloc=None) == -1
    assert bwd(gfeats=None) == -1
    assert bwd(gfeats=null_feats) == -1 and "level 1" in last()
    assert bwd(S=0, gout=None) == 0


def test_python_errors_without_gpu():
    """no CPU fallback: CPU tensors raise, as every operator of the package does"""
    from racformer_amd.msmv import msmv_sampling_v2
    feats = [torch.zeros(2, 3, 4, 6, 8), torch.zeros(2, 3, 2, 3, 8)]
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        msmv_sampling_v2(feats, torch.zeros(2, 4, 5, 3), torch.zeros(2, 4, 5, 2))
