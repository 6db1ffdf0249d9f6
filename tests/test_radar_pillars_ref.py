"""The radar pillar branch without a GPU: the restatement tests/radar_pillars_ref.py on a hand case with literal arrays, the cell
edges of the f8 grid, the padded-row quirk; racformer_amd.radar_pillars' torch-ops route against it; state-dict keys; C-ABI
argument errors."""
import ctypes

import numpy as np
import pytest
import torch

import radar_pillars_ref as R
from racformer_amd import radar_pillars as RP
from racformer_amd import synthetic as syn

HAND_XY = [(0.1, 0.1), (-1.0, 0.1), (0.2, 0.3), (0.3, 0.2), (1.7, 0.0), (1.0, -1.0), (-1.0, -1.0), (-1.2, 0.5)]


def hand_points():
    p = np.zeros((8, 7), np.float32)
    p[:, :2] = np.asarray(HAND_XY, np.float32)
    p[:, 3:] = np.arange(32, dtype=np.float32).reshape(8, 4) + 1          # (tells the points apart)
    return p


def edge_values():
    k = np.arange(-64, 65, dtype=np.float32)
    hi = np.float32(51.2)
    extra = np.asarray([hi, np.nextafter(hi, np.float32(0)), -hi, np.nextafter(-hi, np.float32(-np.inf))], np.float32)
    return k * np.float32(0.8), extra


def edge_points():
    """the 129 edges and the four border values on x (y mid-cell), then the same on y"""
    e, extra = edge_values()
    v = np.concatenate([e, extra])
    p = np.zeros((2 * v.size, 7), np.float32)
    p[:v.size, 0], p[:v.size, 1] = v, 0.4
    p[v.size:, 0], p[v.size:, 1] = 0.4, v
    p[:, 3] = np.arange(p.shape[0])
    return p


def test_hand_case_literal():
    p = hand_points()
    voxels, coors, num, kept = R.hard_voxelize(p, **R.HAND)
    assert coors.tolist() == [[0, 2, 2], [0, 2, 0], [0, 0, 3]]
    assert num.tolist() == [2, 2, 1]
    assert kept == [(0, 0, 0), (1, 1, 0), (2, 0, 1), (5, 2, 0), (7, 1, 1)]      # p3 full, p4 outside, p6 after the cap, p7 kept
    want = np.zeros((3, 2, 7), np.float32)
    want[0, 0], want[0, 1], want[1, 0], want[1, 1], want[2, 0] = p[0], p[2], p[1], p[7], p[5]
    assert np.array_equal(voxels, want)


def test_cell_edges_need_the_true_division():
    e, extra = edge_values()
    true = np.asarray([R.cell_f32(v, -51.2, 0.8) for v in e])
    recip = np.asarray([R.cell_reciprocal_f32(v, -51.2, 0.8) for v in e])
    assert int((true != recip).sum()) == 13
    assert R.cell_f32(extra[0], -51.2, 0.8) >= 128                          # 51.2 itself is outside
    assert R.cell_f32(extra[1], -51.2, 0.8) == 127                          # its predecessor is in the last cell
    assert R.cell_f32(extra[2], -51.2, 0.8) == 0 and R.cell_f32(extra[3], -51.2, 0.8) < 0
    _, coors, _, kept = R.hard_voxelize(edge_points(), **R.F8)
    n = e.size + 4
    dropped = sorted(set(range(2 * n)) - {i for i, _, _ in kept})
    # k = 64 and 51.2 (the same value) and the value below -51.2, on each axis
    assert dropped == [128, 129, 132, n + 128, n + 129, n + 132]


def test_padded_rows_take_part_in_the_max():
    sd = R.make_state_dict(3)
    st = R.Stages(sd, torch.float64, **R.F8)
    p = np.zeros((1, 7), np.float32)
    p[0] = [10.3, -7.1, 0.0, 4.0, -2.0, 1.0, 0.5]
    v, c, n = R.voxelize_batch([p], **R.F8)
    assert v.shape[0] == 1 and int(n[0]) == 1
    got = st.pillar_features(v, c, n)[0]
    floor = torch.relu(st.norm(torch.zeros(1, 64, 1, dtype=torch.float64)))[0, :, 0].detach()      # relu(BN(0))
    g = st.norm.weight / torch.sqrt(st.norm.running_var + st.norm.eps)
    assert torch.allclose(floor, torch.relu(st.norm.bias - st.norm.running_mean * g).detach(), rtol=0, atol=1e-12)
    alone = torch.relu(st.norm(st.linear(st.decorate(v, c, n)[:, :1]).transpose(1, 2)).transpose(1, 2))[0, 0].detach()
    below = alone < floor
    assert bool(below.any()) and bool((~below).any())
    assert torch.allclose(got, torch.maximum(alone, floor), rtol=0, atol=1e-12)
    assert bool((got[below] > alone[below]).all())                          # held up by the padded rows, not by the point
    # a full pillar has no padded row: nothing holds it up
    full = np.repeat(p, 10, axis=0)
    v, c, n = R.voxelize_batch([full], **R.F8)
    assert int(n[0]) == 10 and torch.allclose(st.pillar_features(v, c, n)[0], alone, rtol=0, atol=1e-12)


def poisoned_pillar(slot):
    """SMALL's clouds voxelized, and the same with a NaN in a non-coordinate feature of one in-range point: the first (slot "first")
    or the last real point of a pillar that holds several and has padded rows behind them -> (clean voxels, poisoned voxels, coors,
    num, the pillar's row)"""
    clouds = syn.make_radar_points(4, [0, 1, 40, 300], seed=6, grid=16, edge_fraction=0.2)
    v, c, n = R.voxelize_batch(clouds, zero_z=True, **R.SMALL)
    m = int(torch.nonzero((n >= 3) & (n < R.SMALL["max_num_points"]))[0])
    bad = v.clone()
    bad[m, 0 if slot == "first" else int(n[m]) - 1, 4] = float("nan")
    return v, bad, c, n, m


@pytest.mark.parametrize("slot", ["first", "last"])
def test_nan_point_feature_poisons_its_pillar_alone(slot):
    """torch.max keeps a NaN among a pillar's candidates: all 64 channels of that pillar are NaN, in the features and on the canvas,
    and every other pillar keeps the clean run's bits (the restatement, and the module's torch route)"""
    v, bad, c, n, m = poisoned_pillar(slot)
    st = R.Stages(R.make_state_dict(2), torch.float32, **R.SMALL)
    enc = encoder(R.SMALL, R.make_state_dict(2))
    for feats in (lambda x: st.pillar_features(x, c, n), lambda x: enc.radar_voxel_encoder(x, n, c).detach()):
        clean, got = feats(v), feats(bad)
        assert not bool(torch.isnan(clean).any()) and bool(torch.isnan(got[m]).all())
        others = torch.arange(v.shape[0]) != m
        assert torch.equal(got[others].view(torch.int32), clean[others].view(torch.int32))
    canvas, clean = st.canvas(bad, c, n, 4), st.canvas(v, c, n, 4)
    cell = torch.zeros(clean.shape, dtype=torch.bool)
    cell[int(c[m, 0]), :, int(c[m, 2]), int(c[m, 3])] = True
    assert torch.equal(torch.isnan(canvas), cell) and torch.equal(canvas[~cell], clean[~cell])


RIGS = {
    "hand": (R.HAND, lambda: [hand_points()]),
    "edges": (R.F8, lambda: [edge_points()]),
    "small": (R.SMALL, lambda: [c.numpy() for c in syn.make_radar_points(4, [0, 1, 40, 300], seed=5, grid=16, edge_fraction=0.2)]),
    "small_p3": (dict(R.SMALL, max_num_points=3),
                 lambda: [c.numpy() for c in syn.make_radar_points(4, [0, 1, 40, 300], seed=5, grid=16, edge_fraction=0.2)]),
    "small_cap5": (dict(R.SMALL, max_voxels=5),
                   lambda: [c.numpy() for c in syn.make_radar_points(4, [0, 1, 40, 300], seed=5, grid=16, edge_fraction=0.2)]),
}


@pytest.mark.parametrize("name", sorted(RIGS))
def test_torch_route_voxelization_is_the_oracles(name):
    cfg, clouds = RIGS[name]
    for p in clouds():
        want = R.hard_voxelize(p, **cfg)
        got = RP.hard_voxelize(torch.from_numpy(p), cfg["voxel_size"], cfg["point_cloud_range"], cfg["max_num_points"], cfg["max_voxels"])
        assert got[1].dtype == torch.int32 and got[2].dtype == torch.int32
        assert np.array_equal(got[1].numpy(), want[1]) and np.array_equal(got[2].numpy(), want[2])
        assert np.array_equal(got[0].numpy(), want[0])


def test_synthetic_clouds_cover_the_edge_cases():
    clouds = syn.make_radar_points(3, [0, 300, 300], seed=5, grid=16, edge_fraction=0.2)
    assert clouds[0].shape == (0, 7) and all(torch.equal(a, b) for a, b in zip(clouds, syn.make_radar_points(3, [0, 300, 300], seed=5,
                                                                                                            grid=16, edge_fraction=0.2)))
    p = clouds[1].numpy()
    on_edge = (np.round(p[:, :2] / np.float32(0.8)) * np.float32(0.8) == p[:, :2]).any(axis=1)
    outside = (np.abs(p[:, :2]) >= 6.4).any(axis=1)
    _, _, num, _ = R.hard_voxelize(p, **R.SMALL)
    assert on_edge.sum() >= 30 and outside.sum() >= 10 and num.max() == 10 and (p[:, 2] != 0).any()


def encoder(cfg, sd, fused=True):
    vl = dict(voxel_size=cfg["voxel_size"], point_cloud_range=cfg["point_cloud_range"], max_num_points=cfg["max_num_points"],
              max_voxels=(cfg["max_voxels"], cfg["max_voxels"]), deterministic=False)
    enc = RP.RadarPillarEncoder(radar_voxel_layer=vl, fused=fused)
    enc.load_state_dict(sd)
    return enc.eval()


def test_torch_route_end_to_end_vs_oracle():
    """[B, T, 256, H, W] of the torch-ops route against the float64 restatement, B = 2, T = 2 on the 16 x 16 grid (one cloud
    empty).  Tolerance: 4 x the restatement's own float32-against-float64 error (the project's ratio for a reordered fp32 sum)."""
    sd = R.make_state_dict(11)
    clouds = syn.make_radar_points(4, [0, 40, 300, 120], seed=9, grid=16, edge_fraction=0.2)
    frames = [[clouds[0], clouds[1]], [clouds[2], clouds[3]]]
    before = [c.clone() for c in clouds]
    got = encoder(R.SMALL, sd, fused=False)(frames)
    assert all(torch.equal(a, b) for a, b in zip(clouds, before))          # inputs are not mutated (z stays)
    want, _ = R.forward(sd, R.SMALL, frames, torch.float64)
    f32, _ = R.forward(sd, R.SMALL, frames, torch.float32)
    e_ref = float((f32.double() - want).abs().max())
    assert got.shape == (2, 2, 256, 16, 16) and got.dtype == torch.float32 and got.is_contiguous()
    err = float((got.double() - want).abs().max())
    print(f"torch route: E_ref {e_ref:.3g}, error {err:.3g}")
    assert err <= 4 * e_ref
    # the empty cloud's frame is the stack's response to zeros
    zeros = R.Stages(sd, torch.float64, **R.SMALL).stack_stages(torch.zeros(1, 64, 16, 16, dtype=torch.float64))[-1]
    assert float((got[0, 0].double() - zeros[0]).abs().max()) <= 4 * e_ref


def test_state_dict_keys_and_training_mode():
    enc = RP.RadarPillarEncoder()
    assert sorted(enc.state_dict().keys()) == R.STATE_DICT_KEYS
    assert [n for n, _ in enc.named_children()] == ["radar_voxel_layer", "radar_voxel_encoder", "radar_middle_encoder", "radar_bev_conv"]
    assert tuple(enc.radar_voxel_encoder.pfn_layers[0].linear.weight.shape) == (64, 13)
    enc.train()
    with pytest.raises(RuntimeError, match="training-mode BatchNorm"):
        enc([[torch.zeros(3, 7)]])


def test_capi_argument_errors_need_no_gpu():
    from racformer_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(16)
    geo = (-51.2, -51.2, -5.0, 0.8, 0.8, 8.0, 128, 128, 1)

    def vox(n=8, clouds=1, C=7, P=10, cap=100, g=geo, ptr=one):
        return lib.rac_pillar_voxelize_fwd(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, n, clouds, C, *g, P, cap, None)

    for kw, text in ((dict(C=3), b"point width"), (dict(C=17), b"point width"), (dict(P=33), b"max_num_points"),
                     (dict(P=0), b"max_num_points"), (dict(cap=0), b"max_voxels"), (dict(n=-1), b"n_points"),
                     (dict(g=geo[:3] + (0.0, 0.8, 8.0) + geo[6:]), b"voxel size"), (dict(g=geo[:6] + (0, 128, 1)), b"grid"),
                     (dict(clouds=1 << 20), b"exceed"), (dict(ptr=None), b"null pointer")):
        assert vox(**kw) == -1 and text in lib.rac_last_error(), kw

    def enc(rows=4, clouds=1, C=7, P=10, F=64, H=128, W=128, mul=1.0, canvas=one, image=None, feats=None, wt=one):
        return lib.rac_pillar_encode_fwd(one, one, one, wt, one, None, mul, 0.0, canvas, image, feats, rows, clouds, C, P, F, 0.8, 0.8, 8.0,
                                         -50.8, -50.8, -1.0, H, W, None)

    for kw, text in ((dict(C=20), b"point width"), (dict(P=40), b"max_num_points"), (dict(F=32), b"feature channels"),
                     (dict(H=0), b"H=0"), (dict(mul=-1.0), b"scale constants"), (dict(canvas=None), b"no destination"),
                     (dict(wt=None), b"null pointer"), (dict(canvas=ctypes.c_void_p(20)), b"16-byte aligned")):
        assert enc(**kw) == -1 and text in lib.rac_last_error(), kw
    def cf(xs=one, Cin=64, Cout=256, H=8, mul=1.0, bias=None):
        return lib.rac_conv3x3_relu_cf_fwd(xs, one, bias, None, mul, 0.0, 1.0, one, 1, H, 8, Cin, Cout, None)

    for kw, text in ((dict(Cout=64), b"256 output channels"), (dict(Cin=48), b"Cin=48"), (dict(H=0), b"H=0"), (dict(mul=-2.0), b"scale constants"),
                     (dict(xs=None), b"null pointer"), (dict(bias=ctypes.c_void_p(8)), b"16-byte aligned")):
        assert cf(**kw) == -1 and text in lib.rac_last_error(), kw
    # the two new convolution modes validate like the old ones
    d = _lib.ConvDirect()
    d.mode, d.conv_stride, d.N, d.H, d.W, d.chunks, d.in_chunks_total, d.Cout = _lib.CD_F32_CF_RELU + 1, 1, 1, 8, 8, 2, 2, 64
    for f in ("in_frames", "out_frames", "xpart_frames", "h_prev_frames", "h_out_frames"):
        setattr(d, f, _lib.CdFrames(1, 1, 0))
    assert lib.rac_conv_direct_fwd(ctypes.byref(d), None) == -1 and b"mode=5" in lib.rac_last_error()
    d.mode, d.conv_stride, d.in_img, d.ws, d.out_img = _lib.CD_IMAGE_RELU, 2, one, one, one
    d.out_chunks_total = 2
    assert lib.rac_conv_direct_fwd(ctypes.byref(d), None) == -1 and b"stride 1" in lib.rac_last_error()
    d.mode, d.conv_stride, d.out_f32, d.pixel_map = _lib.CD_F32_CF_RELU, 1, one, one
    assert lib.rac_conv_direct_fwd(ctypes.byref(d), None) == -1 and b"no pixel map" in lib.rac_last_error()
