"""csrc/point_maps.hip on the device against the torch restatement of racformer_amd/point_maps.py run on the CPU, BITWISE: the kernels
and the restatement do the same float32 operations in the same order, and ties in the sort key are decided by the
point index in both, so nothing is excused -- the inputs below hold ties on purpose (depths on a coarse lattice).

Shapes are the smallest at which each path can still go wrong: fewer points than a wave (6 x 10, 5 points), more columns than a
workgroup has lanes (6 x 262), several scan chunks with every column contested (8 x 16, 700 points), ten and more candidates per pixel
(16 x 24, 5 000 lidar points), ranks above 2^17 where a key resolves a depth to 1.56 m only (256 x 704), a downsample of 2, clouds
of 0 / 1 / 300 points with two views each, NaN / inf / p_2 = 0 among the points, a row length that is no multiple of 4 and outputs
that start 4 bytes past a 16-byte boundary.  Every run checks the pads (+0.0), guard words around the outputs and the scratch, and
repeats itself bit for bit."""
import numpy as np
import pytest
import torch

from racformer_amd import point_maps as PM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRID = dict(depth=[1.0, 65.0, 96.0])
GUARD = 64
OUT_SENTINEL, SCRATCH_SENTINEL = 0x7FC0BEEF, 0x5A5A5A5A5A5A5A5A


def camera(hw, yaw, t):
    H, W = hw
    f = W / 2.0
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]])
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.stack([-np.array([-s, c, 0.0]), -np.array([0.0, 0.0, 1.0]), np.array([c, s, 0.0])])
    M = np.eye(4)
    M[:3, :3] = K @ R
    M[:3, 3] = -K @ R @ np.asarray(t, np.float64)
    return M


def cloud(rng, n, M, hw, ds, width=7):
    """n points placed in the map coordinates of view ``M``: pixels shared, a margin outside the map, depths on a 0.5 m lattice from
    0.5 to 75 m (key ties, and drops below lo and beyond hi)."""
    if n == 0:
        return np.zeros((0, width), np.float32)
    H, W = hw[0] // ds, hw[1] // ds
    u = (rng.integers(-1, W + 1, n) + rng.uniform(-0.35, 0.35, n)) * ds
    v = (rng.integers(-1, H + 1, n) + rng.uniform(-0.35, 0.35, n)) * ds
    d = rng.integers(1, 151, n) * 0.5
    xyz = np.linalg.solve(M, np.stack([u * d, v * d, d, np.ones(n)]))[:3].T
    return np.concatenate([xyz, rng.normal(0.0, 8.0, (n, width - 3))], axis=1).astype(np.float32)


def scene(hw, ds, counts, views, seed, width=7):
    """clouds of ``counts`` points, ``views`` views each (view 0 the one the points were placed in, the others turned away a little more
    each) -> (points, offsets, mats table) on the CPU"""
    rng = np.random.default_rng(seed)
    mats, clouds = [], []
    for c, n in enumerate(counts):
        Ms = [camera(hw, 0.03 * c + 0.4 * v, (0.3, 0.1 * v, 0.4)) for v in range(views)]
        mats += Ms
        clouds.append(torch.from_numpy(cloud(rng, n, Ms[0].astype(np.float32).astype(np.float64), hw, ds, width)))
    points, offsets = PM.pack_clouds(clouds)
    return points, offsets, PM.view_table(np.stack(mats))


def guarded(numel, dtype, sentinel, misalign=0):
    """A buffer with GUARD words before and after the ``numel`` that are handed out, everything preset to the sentinel."""
    whole = torch.full((numel + 2 * GUARD + misalign,), sentinel, dtype=torch.int32 if dtype == torch.float32 else torch.int64, device=DEV)
    return whole, whole[GUARD + misalign:GUARD + misalign + numel].view(dtype)


def guards_intact(whole, numel, sentinel, misalign=0):
    return bool((whole[:GUARD + misalign] == sentinel).all()) and bool((whole[GUARD + misalign + numel:] == sentinel).all())


def bits(t):
    return t.contiguous().view(torch.int32)


def run_radar(points, offsets, mats, hw, ds, pad=None, misalign=0, rcs_col=3):
    hm, wm = hw[0] // ds, hw[1] // ds
    hp, wp = pad or (hm, wm)
    n_maps = mats.shape[0]
    dp, od, om = points.to(DEV), offsets.to(DEV), mats.to(DEV)
    outs = []
    for _ in range(2):
        wd, depth = guarded(n_maps * hp * wp, torch.float32, OUT_SENTINEL, misalign)
        wr, rcs = guarded(n_maps * hp * wp, torch.float32, OUT_SENTINEL, misalign)
        words = PM.radar_scratch_words(n_maps, wm)
        ws, scratch = guarded(words, torch.int64, SCRATCH_SENTINEL)
        PM.radar_maps_fwd(dp, od, om, hw, GRID["depth"][0], GRID["depth"][1], ds, (hp, wp), rcs_col, depth=depth, rcs=rcs, scratch=scratch)
        torch.cuda.synchronize()
        assert guards_intact(wd, depth.numel(), OUT_SENTINEL, misalign) and guards_intact(wr, rcs.numel(), OUT_SENTINEL, misalign)
        assert guards_intact(ws, words, SCRATCH_SENTINEL)
        outs.append((depth.view(n_maps, hp, wp).cpu(), rcs.view(n_maps, hp, wp).cpu()))
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(*outs)), "two runs differ"
    want = PM.radar_maps_torch(points, offsets, mats, hw, GRID, ds, (hp, wp), rcs_col)
    for name, g, w in zip(("radar_depth", "radar_rcs"), outs[0], want):
        assert torch.equal(bits(g), bits(w)), (name, int((bits(g) != bits(w)).sum()))
        assert not bits(g[:, hm:]).any() and not bits(g[:, :, wm:]).any(), f"{name}: pads are not +0.0"
    return outs[0]


def run_lidar(points, offsets, mats, hw, ds, pad=None, misalign=0):
    hm, wm = hw[0] // ds, hw[1] // ds
    hp, wp = pad or (hm, wm)
    n_maps = mats.shape[0]
    dp, od, om = points.to(DEV), offsets.to(DEV), mats.to(DEV)
    outs = []
    for _ in range(2):
        wo, out = guarded(n_maps * hp * wp, torch.float32, OUT_SENTINEL, misalign)
        words = PM.lidar_scratch_words(n_maps, hm, wm)
        ws, scratch = guarded(words, torch.int64, SCRATCH_SENTINEL)
        PM.lidar_depth_map_fwd(dp, od, om, hw, GRID["depth"][0], GRID["depth"][1], ds, (hp, wp), out=out, scratch=scratch)
        torch.cuda.synchronize()
        assert guards_intact(wo, out.numel(), OUT_SENTINEL, misalign) and guards_intact(ws, words, SCRATCH_SENTINEL)
        outs.append(out.view(n_maps, hp, wp).cpu())
    assert torch.equal(bits(outs[0]), bits(outs[1])), "two runs differ"
    want = PM.lidar_depth_map_torch(points, offsets, mats, hw, GRID, ds, (hp, wp))
    assert torch.equal(bits(outs[0]), bits(want)), int((bits(outs[0]) != bits(want)).sum())
    assert not bits(outs[0][:, hm:]).any() and not bits(outs[0][:, :, wm:]).any(), "pads are not +0.0"
    return outs[0]


# hw, ds, points per cloud, views, pad, misalign
RADAR = {
    "6x10_5": ((6, 10), 1, [5], 1, None, 0),
    "6x262_40": ((6, 262), 1, [40], 1, None, 0),
    "8x16_700": ((8, 16), 1, [700], 1, None, 0),
    "256x704_2000": ((256, 704), 1, [2000], 1, None, 0),
    "ds2": ((256, 704), 2, [2000], 1, None, 0),
    "clouds_0_1_300": ((12, 20), 1, [0, 1, 300], 2, None, 0),
    "pad_odd_misaligned": ((12, 21), 1, [120, 60], 2, (14, 23), 1),
    "pad_aligned_rows": ((16, 24), 1, [200], 1, (32, 32), 0),
}
LIDAR = {
    "6x10_5": ((6, 10), 1, [5], 1, None, 0),
    "16x24_5000": ((16, 24), 1, [5000], 1, None, 0),
    "256x704_2000": ((256, 704), 1, [2000], 1, None, 0),
    "ds2": ((256, 704), 2, [2000], 1, None, 0),
    "clouds_0_1_300": ((12, 20), 1, [0, 1, 300], 2, None, 0),
    "pad_odd_misaligned": ((12, 21), 1, [120, 60], 2, (14, 23), 1),
}


@pytest.mark.parametrize("name", list(RADAR))
def test_radar_kernel_is_the_restatement(name):
    hw, ds, counts, views, pad, mis = RADAR[name]
    points, offsets, mats = scene(hw, ds, counts, views, seed=len(name) + sum(counts))
    depth, rcs = run_radar(points, offsets, mats, hw, ds, pad, mis)
    if sum(counts) >= 40:
        assert depth.count_nonzero() > 0 and rcs.count_nonzero() > 0
    if name == "8x16_700":
        assert bool((depth[0, 0] != 0).all()), "every column is contested"


@pytest.mark.parametrize("name", list(LIDAR))
def test_lidar_kernel_is_the_restatement(name):
    hw, ds, counts, views, pad, mis = LIDAR[name]
    points, offsets, mats = scene(hw, ds, counts, views, seed=100 + len(name) + sum(counts), width=4)
    out = run_lidar(points, offsets, mats, hw, ds, pad, mis)
    if sum(counts) >= 40:
        assert out.count_nonzero() > 0
    if name == "256x704_2000":
        hm, wm = hw
        assert int(torch.nonzero(out[0].flatten()).max()) > (1 << 17)


def test_special_values():
    """NaN, +-inf and p_2 = 0 among ordinary points: dropped, and the kept count behind them still positions the RCS."""
    hw = (8, 12)
    points, offsets, mats = scene(hw, 1, [90], 2, seed=7)
    odd = torch.tensor([float("nan"), float("inf"), float("-inf")])
    for i in range(0, 90, 4):
        points[i, i // 4 % 3] = odd[i // 12 % 3]
    M = mats[0].view(3, 4).double()
    for i in (1, 9, 33):               # p_2 = 0 exactly: x chosen so that the row-2 products cancel (x M20 = -M23 with y = z = 0)
        points[i, 1:3] = 0
        points[i, 0] = float(-M[2, 3] / M[2, 0])
    run_radar(points, offsets, mats, hw, 1)
    run_lidar(points, offsets, mats, hw, 1)


def test_restatement_on_the_device_is_the_restatement_on_the_cpu():
    hw = (12, 20)
    points, offsets, mats = scene(hw, 1, [150, 40], 2, seed=21)
    on_dev = PM.radar_maps_torch(points.to(DEV), offsets.to(DEV), mats.to(DEV), hw, GRID)
    on_cpu = PM.radar_maps_torch(points, offsets, mats, hw, GRID)
    assert all(torch.equal(bits(a.cpu()), bits(b)) for a, b in zip(on_dev, on_cpu))
    assert torch.equal(bits(PM.lidar_depth_map_torch(points.to(DEV), offsets.to(DEV), mats.to(DEV), hw, GRID).cpu()),
                       bits(PM.lidar_depth_map_torch(points, offsets, mats, hw, GRID)))


def test_public_functions_run_the_kernels_and_one_output_may_be_left_out():
    hw = (12, 20)
    points, offsets, mats = scene(hw, 1, [150, 40], 2, seed=22)
    depth, rcs = PM.radar_maps(points.to(DEV), offsets.to(DEV), mats, hw, GRID, pad_hw=(16, 32))
    want = PM.radar_maps(points, offsets, mats, hw, GRID, pad_hw=(16, 32))
    assert depth.is_cuda and torch.equal(bits(depth.cpu()), bits(want[0])) and torch.equal(bits(rcs.cpu()), bits(want[1]))
    gt = PM.lidar_depth_map(points.to(DEV), offsets.to(DEV), mats, hw, GRID)
    assert torch.equal(bits(gt.cpu()), bits(PM.lidar_depth_map(points, offsets, mats, hw, GRID)))
    only_d, none = PM.radar_maps_fwd(points.to(DEV), offsets.to(DEV), mats.to(DEV), hw, 1.0, 65.0, want=(True, False))
    assert none is None and torch.equal(bits(only_d.cpu()), bits(want[0][:, :12, :20]))
    none, only_r = PM.radar_maps_fwd(points.to(DEV), offsets.to(DEV), mats.to(DEV), hw, 1.0, 65.0, want=(False, True))
    assert none is None and torch.equal(bits(only_r.cpu()), bits(want[1][:, :12, :20]))
    with pytest.raises(RuntimeError, match="rac_point_maps_radar_fwd"):
        PM.radar_maps(points.to(DEV), offsets.to(DEV), mats, hw, dict(depth=[0.0, 65.0, 96.0]))      # lo <= 0: refused on the device route


def test_a_captured_launch_follows_the_points():
    hw = (12, 20)
    points, offsets, mats = scene(hw, 1, [150, 40], 2, seed=23)
    other = scene(hw, 1, [150, 40], 2, seed=24)[0]
    dp, od, om = points.to(DEV), offsets.to(DEV), mats.to(DEV)
    n_maps = mats.shape[0]
    depth, rcs, gt = (torch.empty(n_maps, 12, 20, device=DEV) for _ in range(3))
    rs = torch.empty(PM.radar_scratch_words(n_maps, 20), dtype=torch.int64, device=DEV)
    ls = torch.empty(PM.lidar_scratch_words(n_maps, 12, 20), dtype=torch.int64, device=DEV)

    def launch():
        PM.radar_maps_fwd(dp, od, om, hw, 1.0, 65.0, depth=depth, rcs=rcs, scratch=rs)
        PM.lidar_depth_map_fwd(dp, od, om, hw, 1.0, 65.0, out=gt, scratch=ls)

    launch()                               # (warm-up outside the capture: the module is loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for pts in (other, points):
        dp.copy_(pts.to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        want = PM.radar_maps_torch(pts, offsets, mats, hw, GRID) + (PM.lidar_depth_map_torch(pts, offsets, mats, hw, GRID),)
        assert all(torch.equal(bits(g.cpu()), bits(w)) for g, w in zip((depth, rcs, gt), want))
    assert not torch.equal(PM.radar_maps_torch(other, offsets, mats, hw, GRID)[0], PM.radar_maps_torch(points, offsets, mats, hw, GRID)[0])
