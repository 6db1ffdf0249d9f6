"""racformer_amd/point_maps.py without a GPU: the torch restatement of rules 1-6 against the maps the reference's own
``RadarPointToMultiViewDepth`` / ``PointToMultiViewDepth`` made (tests/golden/point_maps_small.npz, written by
tests/golden/gen_golden_point_maps.py on inputs where the reference's result depends neither on rounding nor on the order of tied
keys), the C-ABI's refusals, ``pad_hw`` and the table helpers.

Against the fixture: the occupied positions are identical; ``radar_rcs`` is bitwise identical (a copy of an input value); a depth
is the winning point's ``p_2``, a four-term float32 sum the reference's matmul may add in another order, so it may differ by
``4 * 2^-24 * (|x M20| + |y M21| + |z M22| + |M23|)`` of that point (each of the three additions and the products' roundings stay
below 2^-24 of the sum of magnitudes) and by no more.  No pixel is excused."""
import ctypes
import os

import numpy as np
import pytest
import torch

from racformer_amd import _lib, point_maps as PM

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = ["a", "b", "c", "d"]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "point_maps_small.npz"))


def case(golden, name):
    g = {k.split(":", 1)[1]: golden[k] for k in golden.files if k.startswith(name + ":")}
    g["points"], g["offsets"] = torch.from_numpy(g["points"]), torch.from_numpy(g["offsets"])
    g["grid"] = dict(depth=[float(g["depth"][0]), float(g["depth"][1]), 96.0])
    g["hw"], g["ds"], g["n_views"] = tuple(int(v) for v in g["hw"]), int(g["ds"]), int(g["n_views"])
    return g


def depth_bound(points, mats, winner, map_of):
    """The bound of the module docstring for the points ``winner`` (indices into ``points``) under the maps' matrices."""
    p, m = points[winner].double(), mats[map_of].double()
    return 4 * 2.0 ** -24 * ((p[:, 0] * m[:, 8]).abs() + (p[:, 1] * m[:, 9]).abs() + (p[:, 2] * m[:, 10]).abs() + m[:, 11].abs())


@pytest.mark.parametrize("name", CASES)
def test_radar_maps_against_the_reference(golden, name):
    g = case(golden, name)
    mats = PM.view_table(g["lidar2img"])
    winners = []
    depth, rcs = PM.radar_maps_torch(g["points"], g["offsets"], mats, g["hw"], g["grid"], g["ds"], winners=winners)
    hm, wm = g["hw"][0] // g["ds"], g["hw"][1] // g["ds"]
    assert tuple(depth.shape) == tuple(rcs.shape) == (mats.shape[0], hm, wm)
    idx = torch.from_numpy(g["radar_idx"])
    assert torch.equal(torch.nonzero(depth.flatten()).flatten(), idx), "occupied positions of radar_depth"
    assert torch.equal(torch.nonzero(rcs.flatten()).flatten(), idx), "occupied positions of radar_rcs"
    assert torch.equal(rcs.flatten()[idx], torch.from_numpy(g["radar_rcs"])), "radar_rcs is a copy of an input value"
    if idx.numel() == 0:
        return
    map_of, col_of = idx // (hm * wm), idx % wm
    win = torch.stack(winners)[map_of, col_of]
    assert int(win.min()) >= 0
    err = (depth.flatten()[idx].double() - torch.from_numpy(g["radar_depth"]).double()).abs()
    bound = depth_bound(g["points"], mats, win, map_of)
    print(f"radar {name}: {idx.numel()} elements, largest depth difference {float(err.max()):.3g}, smallest bound {float(bound.min()):.3g}")
    assert bool((err <= bound).all()), (float(err.max()), float(bound.min()))


@pytest.mark.parametrize("name", CASES)
def test_lidar_map_against_the_reference(golden, name):
    g = case(golden, name)
    N = g["n_views"]
    mats = PM.view_table(g["lidar2img"][:N])
    pts, off = g["points"][: int(g["offsets"][1])], g["offsets"][:2].clone()
    winners = []
    out = PM.lidar_depth_map_torch(pts, off, mats, g["hw"], g["grid"], g["ds"], winners=winners)
    hm, wm = g["hw"][0] // g["ds"], g["hw"][1] // g["ds"]
    idx = torch.from_numpy(g["lidar_idx"])
    assert tuple(out.shape) == (N, hm, wm)
    assert torch.equal(torch.nonzero(out.flatten()).flatten(), idx), "occupied positions of gt_depth"
    assert idx.numel() > 0
    win = torch.stack(winners).flatten()[idx]
    err = (out.flatten()[idx].double() - torch.from_numpy(g["lidar_depth"]).double()).abs()
    bound = depth_bound(pts, mats, win, idx // (hm * wm))
    print(f"lidar {name}: {idx.numel()} pixels, largest depth difference {float(err.max()):.3g}, smallest bound {float(bound.min()):.3g}")
    assert bool((err <= bound).all()), (float(err.max()), float(bound.min()))


def test_the_fixture_shows_the_rcs_quirk(golden):
    """Somewhere the value written is not the winner's own RCS (rule 5) -- otherwise the fixture could not tell the two readings apart."""
    differs = 0
    for name in CASES:
        g = case(golden, name)
        winners = []
        _, rcs = PM.radar_maps_torch(g["points"], g["offsets"], PM.view_table(g["lidar2img"]), g["hw"], g["grid"], g["ds"], winners=winners)
        for m, w in enumerate(winners):
            cols = torch.nonzero(w >= 0).flatten()
            differs += int((rcs[m, 0, cols] != g["points"][w[cols], PM.RCS_COLUMN]).sum())
    assert differs > 0


def test_public_functions_take_the_restatement_on_cpu_and_pad(golden):
    g = case(golden, "b")
    mats = PM.view_table(g["lidar2img"])
    plain = PM.radar_maps(g["points"], g["offsets"], g["lidar2img"], g["hw"], g["grid"])            # (matrices, not a table: converted)
    want = PM.radar_maps_torch(g["points"], g["offsets"], mats, g["hw"], g["grid"])
    assert all(torch.equal(a, b) for a, b in zip(plain, want))
    H, W = g["hw"]
    padded = PM.radar_maps(g["points"], g["offsets"], mats, g["hw"], g["grid"], pad_hw=(H + 4, W + 3))
    for p, w in zip(padded, want):
        assert tuple(p.shape) == (mats.shape[0], H + 4, W + 3) and torch.equal(p[:, :H, :W], w)
        assert not p[:, H:].any() and not p[:, :, W:].any() and not torch.signbit(p[:, H:]).any() and not torch.signbit(p[:, :, W:]).any()
    lid = PM.lidar_depth_map(g["points"], g["offsets"], mats, g["hw"], g["grid"], pad_hw=(H + 1, W + 5))
    assert torch.equal(lid[:, :H, :W], PM.lidar_depth_map_torch(g["points"], g["offsets"], mats, g["hw"], g["grid"])) and not lid[:, H:].any()
    with pytest.raises(ValueError, match="smaller than the map"):
        PM.radar_maps(g["points"], g["offsets"], mats, g["hw"], g["grid"], pad_hw=(H - 1, W))
    with pytest.raises(ValueError, match="downsample"):
        PM.radar_maps(g["points"], g["offsets"], mats, g["hw"], g["grid"], downsample=0)
    with pytest.raises(ValueError, match="view matrices"):
        PM.radar_maps(g["points"], g["offsets"], mats[:3], g["hw"], g["grid"])
    with pytest.raises(ValueError, match="RCS column"):
        PM.radar_maps(g["points"], g["offsets"], mats, g["hw"], g["grid"], rcs_col=7)


def test_special_values_are_dropped():
    """NaN, +-inf and p_2 = 0 fail the comparisons; a point behind the camera has d < lo; -0.0 coordinates are pixel 0."""
    M = np.eye(4, dtype=np.float32)           # u = x / z, v = y / z, d = z
    pts = torch.tensor([[float("nan"), 0, 5, 1], [0, float("inf"), 5, 2], [1, 1, 0, 3], [0, 0, float("inf"), 4], [2, 1, -5, 5],
                        [-0.0, -0.0, 7, 6], [float("-inf"), 0, 5, 7], [8, 4, 2, 8]], dtype=torch.float32)
    off = torch.tensor([0, 8], dtype=torch.int32)
    grid = dict(depth=[1.0, 65.0, 96.0])
    depth, rcs = PM.radar_maps_torch(pts, off, [M], (4, 6), grid)
    lid = PM.lidar_depth_map_torch(pts, off, [M], (4, 6), grid)
    assert torch.nonzero(lid[0]).tolist() == [[0, 0], [2, 4]] and float(lid[0, 0, 0]) == 7.0 and float(lid[0, 2, 4]) == 2.0
    assert torch.nonzero(depth[0, 0]).flatten().tolist() == [0, 4]
    assert rcs[0, 0, [0, 4]].tolist() == [1.0, 2.0]          # positions 0 and 1 among the kept points: the RCS of points 0 and 1


def test_meta_view_table_orders_samples_then_frames():
    metas = [dict(lidar2img=[np.full((4, 4), 10 * b + i, np.float64) for i in range(6)]) for b in range(2)]
    t = PM.meta_view_table(metas, 3)
    assert tuple(t.shape) == (12, 12) and t.dtype == torch.float32 and t[:, 0].tolist() == [0, 1, 2, 3, 4, 5, 10, 11, 12, 13, 14, 15]
    assert PM.meta_view_table(metas, 3, frames=1)[:, 0].tolist() == [0, 1, 2, 10, 11, 12]
    with pytest.raises(ValueError):
        PM.meta_view_table(metas, 3, frames=3)


# ------------------------------------------------------------------------------------------------ refusals before any HIP call
def radar_call(**over):
    a = dict(points=8, offsets=8, mats=8, depth=8, rcs=8, scratch=8, words=1 << 40, n_points=10, n_clouds=1, n_views=1, C=7, rcs_col=3,
             H=16, W=32, Hp=16, Wp=32, ds=1, lo=1.0, hi=65.0)
    a.update(over)
    p = lambda v: ctypes.c_void_p(v)       # noqa: E731
    return _lib.lib().rac_point_maps_radar_fwd(p(a["points"]), p(a["offsets"]), p(a["mats"]), p(a["depth"]), p(a["rcs"]), p(a["scratch"]),
                                               a["words"], a["n_points"], a["n_clouds"], a["n_views"], a["C"], a["rcs_col"], a["H"], a["W"],
                                               a["Hp"], a["Wp"], a["ds"], a["lo"], a["hi"], None)


def lidar_call(**over):
    a = dict(points=8, offsets=8, mats=8, out=8, scratch=8, words=1 << 40, n_points=10, n_clouds=1, n_views=1, C=4, H=16, W=32, Hp=16, Wp=32,
             ds=1, lo=1.0, hi=65.0)
    a.update(over)
    p = lambda v: ctypes.c_void_p(v)       # noqa: E731
    return _lib.lib().rac_point_maps_lidar_fwd(p(a["points"]), p(a["offsets"]), p(a["mats"]), p(a["out"]), p(a["scratch"]), a["words"],
                                               a["n_points"], a["n_clouds"], a["n_views"], a["C"], a["H"], a["W"], a["Hp"], a["Wp"], a["ds"],
                                               a["lo"], a["hi"], None)


ARG, UNSUPPORTED = -1, -2


@pytest.mark.parametrize("call", [radar_call, lidar_call])
@pytest.mark.parametrize("over, rc", [
    (dict(points=None), ARG), (dict(offsets=None), ARG), (dict(mats=None), ARG), (dict(scratch=None), ARG),
    (dict(ds=0), ARG), (dict(ds=-2), ARG), (dict(Hp=15), ARG), (dict(Wp=31), ARG), (dict(words=3), ARG), (dict(C=2), ARG),
    (dict(scratch=12), ARG), (dict(H=1, W=1, ds=2), ARG),
    (dict(H=512, W=513, Hp=512, Wp=513), UNSUPPORTED),           # more than 2^18 pixels
    (dict(H=1024, W=1026, Hp=512, Wp=513, ds=2), UNSUPPORTED),
    (dict(hi=99.5), UNSUPPORTED), (dict(lo=0.0), UNSUPPORTED), (dict(lo=-1.0), UNSUPPORTED),
    (dict(n_points=1 << 20), UNSUPPORTED),
    (dict(H=4097, W=8, Hp=4097, Wp=8), UNSUPPORTED),
])
def test_refusals_need_no_gpu(call, over, rc):
    assert call(**over) == rc, _lib.lib().rac_last_error()
    assert _lib.lib().rac_last_error()


def test_refusals_of_the_outputs_and_the_rcs_column():
    assert radar_call(depth=None, rcs=None) == ARG and b"neither" in _lib.lib().rac_last_error()
    assert radar_call(rcs_col=7) == ARG and radar_call(rcs_col=-1) == ARG
    assert lidar_call(out=None) == ARG
    assert radar_call(depth=10) == ARG          # (2 bytes off)
