"""The float64 reference of the backward tests (tests/test_backward_f64_gpu.py) pinned on its own, on CPU: finite-difference
gradchecks of the oracle's pure-torch gathers and of bev_pool_v2, agreement with the C oracle's float64 instance, the view
pick at halfway values (round half away from zero, as C ``round``), float32 coordinates on request, and bit-identity of the
oracle's float32 results with what it computed before it learned float64 (tests/golden/oracle_f32_pin.npz)."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import restate as R


def _away_from_grid(x, scale, shift=0.0, margin=0.02):
    """True when x * scale - shift lies at least `margin` away from every integer (finite differences stay on one tap set)."""
    y = x * scale - shift
    return bool(((y - torch.floor(y)).clamp(margin, 1 - margin) == (y - torch.floor(y))).all())


def _msmv_case(seed, S=2, N=3, Q=2, P=3, C=2, hws=((5, 7), (3, 4))):
    g = torch.Generator().manual_seed(seed)
    feats = [torch.randn(S, N, h, w, C, generator=g, dtype=torch.float64) for h, w in hws]
    loc = torch.rand(S, Q, P, 3, generator=g, dtype=torch.float64) * 1.1 - 0.05
    loc[..., 2] = torch.randint(0, N, (S, Q, P), generator=g).double() / (N - 1)
    w = torch.rand(S, Q, P, len(hws), generator=g, dtype=torch.float64)
    return feats, loc, w


def _msda_case(seed, bs=2, Q=3, heads=2, dim=3, P=2, shapes=((4, 5), (2, 3), (1, 4)), gap=3):
    g = torch.Generator().manual_seed(seed)
    starts, k = [], gap                                       # non-zero starts, a gap before the first level
    for h, w in shapes:
        starts.append(k)
        k += h * w + 1                                        # and one unused key between levels
    keys = k + 2
    value = torch.randn(bs, keys, heads, dim, generator=g, dtype=torch.float64)
    loc = torch.rand(bs, Q, heads, len(shapes), P, 2, generator=g, dtype=torch.float64) * 1.2 - 0.1
    attn = torch.rand(bs, Q, heads, len(shapes), P, generator=g, dtype=torch.float64)
    return value, [list(s) for s in shapes], starts, loc, attn


def test_gradcheck_msmv_gather_torch():
    for seed in range(100):
        feats, loc, w = _msmv_case(seed)
        if all(_away_from_grid(loc[..., 0], s) for s in (6, 3)) and all(_away_from_grid(loc[..., 1], s) for s in (4, 2)):
            break
    else:
        pytest.fail("no seed keeps the locations off the grid")
    ins = [f.requires_grad_() for f in feats] + [loc.requires_grad_(), w.requires_grad_()]
    L = len(feats)
    assert torch.autograd.gradcheck(lambda *a: R.msmv_gather_torch(list(a[:L]), a[L], a[L + 1]), ins, eps=1e-6, atol=1e-8)


def test_gradcheck_msda_torch():
    for seed in range(100):
        value, shapes, starts, loc, attn = _msda_case(seed)
        ok = all(_away_from_grid(loc[..., l, :, i], shapes[l][1 - i], 0.5, margin=0.005)
                 for l in range(len(shapes)) for i in (0, 1))
        if ok:
            break
    else:
        pytest.fail("no seed keeps the locations off the grid")
    ins = [value.requires_grad_(), loc.requires_grad_(), attn.requires_grad_()]
    assert torch.autograd.gradcheck(lambda v, l, a: R.msda_torch(v, shapes, starts, l, a), ins, eps=1e-6, atol=1e-8)


def test_gradcheck_bev_pool_v2():
    g = torch.Generator().manual_seed(4)
    depth = torch.rand(1, 1, 3, 2, 2, generator=g, dtype=torch.float64)     # 12 depth entries
    feat = torch.randn(1, 1, 2, 2, 5, generator=g, dtype=torch.float64)     # 4 feature cells, c = 5
    rd = torch.arange(12, dtype=torch.int32)
    rf = rd % 4
    rb = torch.tensor([0, 0, 0, 2, 2, 3, 3, 3, 3, 5, 7, 7], dtype=torch.int32)   # sorted, ragged, empty cells between
    starts, lengths = torch.tensor([0, 3, 5, 9, 10], dtype=torch.int32), torch.tensor([3, 2, 4, 1, 2], dtype=torch.int32)
    f = lambda d, x: R.bev_pool_v2(d, x, rd, rf, rb, (1, 1, 2, 4, 5), starts, lengths)
    assert f(depth, feat).dtype == torch.float64
    assert torch.autograd.gradcheck(f, [depth.requires_grad_(), feat.requires_grad_()], eps=1e-6, atol=1e-8)


@pytest.fixture(scope="module")
def clib():
    if R._clib() is None:
        pytest.fail("C oracle (oracle/libgather_ref.so) not built")
    return R._clib()


def _edge_uv(H, W):
    """normalised (u, v) pairs whose align_corners=True coordinates hit the edges (H-1, W-1 powers of two: exact)"""
    cases = [(0.0, 0.0), (1.0, 1.0), (0.25, 0.5), (0.5 / (W - 1) * -1, 0.3), (0.3, -0.5 / (H - 1)),
             (-1.0 / (W - 1), 0.4), (0.4, -1.0 / (H - 1)), (W / (W - 1), 0.6), (0.6, H / (H - 1)),
             (float(np.nextafter(np.float32(W / (W - 1)), np.float32(0))), 0.7), (1e-7, 1 - 1e-7)]
    return torch.tensor(cases, dtype=torch.float32)


def test_msmv_float64_matches_c_f64(clib):
    feats, loc, w = _msmv_case(7, S=3, N=4, Q=5, P=11, C=6, hws=((9, 17), (5, 3), (1, 9), (9, 1)))
    loc = loc.float().double()
    uv = _edge_uv(9, 17).double()
    loc[0, 0, :uv.shape[0], :2] = uv
    out = R.msmv_gather_torch(feats, loc, w)
    assert out.dtype == torch.float64
    ref = R.msmv_gather(feats, loc, w)                      # the C text's `_f64` instance
    assert ref.dtype == torch.float64
    assert float((out - ref).abs().max()) <= 1e-13 * max(1.0, float(ref.abs().max()))


def test_msda_float64_matches_c_f64(clib):
    value, shapes, starts, loc, attn = _msda_case(8, bs=2, Q=4, heads=3, dim=5, P=4, shapes=((8, 4), (4, 2), (1, 3), (2, 1)))
    out = R.msda_torch(value, shapes, starts, loc, attn)
    assert out.dtype == torch.float64                       # accumulated in float64, not into a float32 buffer
    ref = R.msda(value, shapes, starts, loc, attn)
    assert ref.dtype == torch.float64
    assert float((out - ref).abs().max()) <= 1e-13 * max(1.0, float(ref.abs().max()))
    # the float32 accumulator of old would have lost this
    assert float((out - R.msda_torch(value.float(), shapes, starts, loc.float(), attn.float()).double()).abs().max()) > 1e-9


def _halfway_z(N):
    """(k, z) with float32 z and fl32(z * (N-1)) = k + 1/2 exactly, for the k in 0 .. N-2 where such a z exists"""
    out = []
    for k in range(N - 1):
        z0 = np.float32((k + 0.5) / (N - 1))
        for z in (z0, np.nextafter(z0, np.float32(0)), np.nextafter(z0, np.float32(1))):
            if z * np.float32(N - 1) == np.float32(k + 0.5):
                out.append((k, float(z)))
                break
    return out


@pytest.mark.parametrize("N", [2, 4, 6])
def test_view_pick_at_halfway_values(clib, N):
    """torch and C oracles (float32, float64 with float32 coordinates) pick the same camera as C round: k + 1/2 -> k + 1."""
    ks, zs = zip(*_halfway_z(N))
    assert len(zs) >= (N - 1) // 2 + 1                      # the ties exist in float32 at every N tested
    S, Q, P, C = 1, 1, len(zs), 1
    feat = torch.arange(N, dtype=torch.float32).reshape(1, N, 1, 1, 1).expand(S, N, 2, 2, C).contiguous()
    loc = torch.zeros(S, Q, P, 3)
    loc[..., 0], loc[..., 1] = 0.5, 0.5
    loc[0, 0, :, 2] = torch.tensor(zs)
    w = torch.ones(S, Q, P, 1)
    want = torch.tensor(ks, dtype=torch.float32) + 1       # half away from zero; torch.round would give the even one
    got32 = R.msmv_gather_torch([feat], loc, w)[0, 0, 0]
    c32 = R.msmv_gather([feat], loc, w)[0, 0, 0]
    got64 = R.msmv_gather_torch([feat.double()], loc.double(), w.double(), f32_coords=True)[0, 0, 0]
    assert torch.equal(got32, want) and torch.equal(c32, want) and torch.equal(got64, want.double())


def test_f32_coords_reproduce_float32_products():
    """with f32_coords a float64 coordinate equals the float32 one bit for bit, and its derivative is the exact scale"""
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(4096, generator=g) * 1.3 - 0.15).double().requires_grad_()
    for scale, shift in ((7, 0), (16, 0), (13, 0.5), (8, 0.5), (1, 0.5)):
        y = R._coord(x, scale, shift, True)
        y32 = x.detach().float() * scale - shift if shift else x.detach().float() * scale
        assert torch.equal(y.detach(), y32.double())
        (gx,) = torch.autograd.grad(y.sum(), x)
        assert torch.equal(gx, torch.full_like(gx, float(scale)))
    # a product that rounds onto an integer in float32 but not in float64 picks the float32 taps
    v32 = np.float32(3 / 7)
    assert v32 * np.float32(7) == 3 and float(v32) * 7 != 3
    v = torch.tensor([float(v32)], dtype=torch.float64)
    assert float(R._coord(v, 7, 0, True)) == 3 and float(R._coord(v, 7, 0, False)) != 3


def test_float32_results_bit_identical_to_the_pin(golden_dir):
    sys.path.insert(0, golden_dir)
    try:
        from gen_oracle_f32_pin import pinned_outputs
    finally:
        sys.path.remove(golden_dir)
    pin = np.load(os.path.join(golden_dir, "oracle_f32_pin.npz"))
    now = pinned_outputs(R, golden_dir)
    assert sorted(now) == sorted(pin.files)
    for k in pin.files:
        assert now[k].dtype == np.float32 and np.array_equal(now[k], pin[k]), k
