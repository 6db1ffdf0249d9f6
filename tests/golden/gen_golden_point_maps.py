#!/usr/bin/env python3
"""Golden vectors of the point maps: runs the REFERENCE's own ``RadarPointToMultiViewDepth.load_offline`` and
``PointToMultiViewDepth.__call__`` (loaders/pipelines/loading.py:470-600) on CPU and writes a data-only fixture next to this script.
Run in the build container only (needs the reference tree):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_point_maps.py

``loading.py`` is loaded by path under stub modules for everything it imports at module level and never touches on this path (mmcv,
mmdet, mmdet3d.core.points, loaders.nuscenes_dataset, cv2, matplotlib.pyplot, pyquaternion).  ``load_offline`` slices six views per
frame, so it is called once per frame with that frame's views.

  point_maps_small.npz, per case ``name`` (keys ``name:...``):
      hw [2] (the image), ds, depth [2] (lo, hi), n_views, points [n, 7] float32 and offsets int32 [T + 1] (the radar clouds of the T
      frames, packed; cloud 0 is also the lidar cloud), lidar2img [T * n_views, 4, 4] float32,
      radar_idx int64 / radar_depth / radar_rcs float32: flat indices into [T * n_views, hm, wm] where the reference's radar_depth
      is not 0, and both maps' values there (radar_rcs is not 0 anywhere else either: asserted),
      lidar_idx / lidar_depth: the same for gt_depth [n_views, hm, wm] of cloud 0 with frame 0's views.
  cases: a 6 x 10, b 12 x 20, c 32 x 64 (a 64 x 128 image at ds = 2) -- each 2 frames x 2 views, frame 1's second view facing away
  (all of its points dropped), frame 1's cloud of case a empty --, d one 256 x 704 map of 2 000 points (ranks above 2^17).

The reference's ``argsort`` is not stable and its projection is a library matmul, so inputs are redrawn (the seed is advanced) until
the reference's result cannot depend on either, and every condition is ASSERTED on what is written: in float64, every point that is
kept or within a pixel / 1e-3 m of being kept has u / ds and v / ds at least 1e-3 from a half-integer and d at least 1e-3 from lo
and hi; inside a pixel no two kept points' float32 keys are closer than 4 ulp of the key.  The cases together must show: a column
with winners in two or more rows, a pixel with two or more candidates, a winner whose position among the kept points differs from
its index (the RCS quirk), and a dropped point of each kind (left, right, above, below, nearer than lo, at or beyond hi)."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("RACFORMER_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True

DEPTH = (1.0, 65.0)
CASES = {
    "a": dict(hw=(6, 10), ds=1, n=(14, 0), frames=2, views=2),
    "b": dict(hw=(12, 20), ds=1, n=(40, 25), frames=2, views=2),
    "c": dict(hw=(64, 128), ds=2, n=(160, 90), frames=2, views=2),
    "d": dict(hw=(256, 704), ds=1, n=(2000,), frames=1, views=1),
}


def load_loading():
    class Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("mmcv")
    mod("mmcv.runner", get_dist_info=lambda: (0, 1))
    mod("mmcv.parallel", DataContainer=object)
    mod("mmdet")
    mod("mmdet.datasets")
    mod("mmdet.datasets.builder", PIPELINES=Registry())
    mod("mmdet.datasets.pipelines", LoadAnnotations=type("LoadAnnotations", (), {}), LoadImageFromFile=type("LoadImageFromFile", (), {}))
    mod("mmdet3d")
    mod("mmdet3d.core")
    mod("mmdet3d.core.points", BasePoints=object, get_points_type=None)
    mod("loaders")
    mod("loaders.nuscenes_dataset", get_nu_radar=None)
    mod("cv2")
    mod("matplotlib")
    mod("matplotlib.pyplot")
    mod("pyquaternion", Quaternion=object)
    spec = importlib.util.spec_from_file_location("rac_reference_loading", os.path.join(REF_ROOT, "loaders", "pipelines", "loading.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ------------------------------------------------------------------------------------------------ inputs
def camera(hw, yaw, t):
    """float64 lidar2img of a pinhole camera at ``t`` looking along the lidar frame's x axis turned by ``yaw`` (90 degrees wide)."""
    H, W = hw
    f = W / 2.0
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]])
    c, s = np.cos(yaw), np.sin(yaw)
    fwd, left, up = np.array([c, s, 0.0]), np.array([-s, c, 0.0]), np.array([0.0, 0.0, 1.0])
    R = np.stack([-left, -up, fwd])                     # camera axes: x right, y down, z forward
    M = np.eye(4)
    M[:3, :3] = K @ R
    M[:3, 3] = -K @ R @ np.asarray(t, np.float64)
    return M


def draw_cloud(rng, n, M, hw, ds):
    """n points [n, 7] chosen in the first view's map coordinates, so that pixels are shared and every kind of drop occurs."""
    if n == 0:
        return np.zeros((0, 7), np.float32)
    H, W = hw[0] // ds, hw[1] // ds
    cells = max(3, min(n // 3, H * W // 4))
    px = rng.integers(-2, W + 2, cells) + rng.uniform(-0.3, 0.3, cells)       # (pixel centres +- 0.3: away from the half-integers)
    py = rng.integers(-1, H + 1, cells) + rng.uniform(-0.3, 0.3, cells)
    px[: max(2, cells // 4)] = px[0]                                           # one crowded column, several rows
    pick = rng.integers(0, cells, n)
    u, v = px[pick] * ds, py[pick] * ds
    seen, occ = {}, np.zeros(n)
    for i, key in enumerate(zip(np.rint(px[pick]).tolist(), np.rint(py[pick]).tolist())):
        occ[i] = seen[key] = seen.get(key, -1) + 1
    d = rng.uniform(0.2, 2.2, n) + 9.0 * occ             # a pixel's candidates 7 m or more apart: 4 ulp of a key near 2^18 are 6.25 m
    d = np.where(rng.uniform(0, 1, n) < 0.08, rng.uniform(66.0, 80.0, n), d)
    cam = np.stack([u * d, v * d, d, np.ones(n)])
    xyz = np.linalg.solve(M, cam)[:3].T
    rest = rng.normal(0.0, 8.0, (n, 4))
    return np.concatenate([xyz, rest], axis=1).astype(np.float32)


def make_case(cfg, seed):
    rng = np.random.default_rng(seed)
    T, N = cfg["frames"], cfg["views"]
    mats = []
    for t in range(T):
        for v in range(N):
            yaw = 0.02 * t if v == 0 else (np.pi if t == T - 1 else 0.35)
            mats.append(camera(cfg["hw"], yaw, (0.3 + 0.1 * v, 0.05 * t, 0.4)))
    mats = np.stack(mats).astype(np.float32)
    clouds = [draw_cloud(rng, cfg["n"][t], mats[t * N].astype(np.float64), cfg["hw"], cfg["ds"]) for t in range(T)]
    return clouds, mats


# ------------------------------------------------------------------------------------------------ the conditions
def examine(cloud, M, hw, ds):
    """One cloud, one view, in float64 and (the keys) float32 -> (ok, facts): ok False when the reference's result could depend on
    rounding or on the order of tied keys."""
    lo, hi = DEPTH
    H, W = hw[0] // ds, hw[1] // ds
    facts = dict(rows=False, crowd=False, quirk=False, left=False, right=False, above=False, below=False, near=False, far=False)
    if len(cloud) == 0:
        return True, facts
    p = cloud[:, :3].astype(np.float64) @ M[:3, :3].astype(np.float64).T + M[:3, 3].astype(np.float64)
    d = p[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u, v = p[:, 0] / d / ds, p[:, 1] / d / ds
    cx, cy = np.rint(u), np.rint(v)
    near_kept = (cx >= -1) & (cx <= W) & (cy >= -1) & (cy <= H) & (d > lo - 1e-3) & (d < hi + 1e-3)
    half = lambda a: np.abs(a - np.floor(a) - 0.5)      # noqa: E731
    if np.any(near_kept & ((half(u) < 1e-3) | (half(v) < 1e-3) | (np.abs(d - lo) < 1e-3) | (np.abs(d - hi) < 1e-3))):
        return False, facts
    kept = (cx >= 0) & (cx < W) & (cy >= 0) & (cy < H) & (d >= lo) & (d < hi)
    front = (d >= lo) & (d < hi)
    facts.update(left=bool(np.any(front & (cx < 0))), right=bool(np.any(front & (cx >= W))), above=bool(np.any(front & (cy < 0))),
                 below=bool(np.any(front & (cy >= H))), near=bool(np.any((d < lo) & (d > 0))), far=bool(np.any(d >= hi)))
    idx = np.nonzero(kept)[0]
    if len(idx) == 0:
        return True, facts
    rank = (cx[idx] + cy[idx] * W).astype(np.float32)
    key = rank + (d[idx].astype(np.float32) / np.float32(100.0))
    winners = {}
    for r in np.unique(rank):
        here = np.nonzero(rank == r)[0]
        ks = np.sort(key[here])
        if len(ks) > 1:
            facts["crowd"] = True
            if np.any(np.diff(ks) < 4 * np.spacing(ks[:-1])):
                return False, facts
        winners[int(r)] = here[np.argmin(key[here])]            # position among the kept points
    cols = {}
    for r, s in winners.items():
        cols.setdefault(r % W, []).append(r // W)
        if idx[s] != s:
            facts["quirk"] = True
    facts["rows"] = any(len(set(rows)) > 1 for rows in cols.values())
    return True, facts


class Cloud:
    def __init__(self, tensor):
        self.tensor = tensor


def reference_maps(L, clouds, mats, cfg):
    T, N = cfg["frames"], cfg["views"]
    grid = dict(depth=[DEPTH[0], DEPTH[1], 96.0])
    img = np.zeros(cfg["hw"] + (3,), np.float32)
    radar = L.RadarPointToMultiViewDepth(grid, downsample=cfg["ds"])
    depth, rcs = [], []
    for t in range(T):
        res = radar.load_offline(dict(radar_points=[Cloud(torch.from_numpy(clouds[t]))], img=[img],
                                      lidar2img=[m for m in mats[t * N:(t + 1) * N]]))
        depth.append(res["radar_depth"])
        rcs.append(res["radar_rcs"])
    lidar = L.PointToMultiViewDepth(grid, downsample=cfg["ds"])
    gt = lidar(dict(points=Cloud(torch.from_numpy(clouds[0])), img=[img], lidar2img=[m for m in mats]))["gt_depth"][:N]
    return torch.cat(depth).numpy(), torch.cat(rcs).numpy(), gt.numpy()


def main():
    L = load_loading()
    out, shown = {}, {}
    for name, cfg in CASES.items():
        T, N = cfg["frames"], cfg["views"]
        for seed in range(1000 * (ord(name) - 96), 1000 * (ord(name) - 96) + 400):
            clouds, mats = make_case(cfg, seed)
            checks = [examine(clouds[t], mats[t * N + v], cfg["hw"], cfg["ds"]) for t in range(T) for v in range(N)]
            checks += [examine(clouds[0], mats[v], cfg["hw"], cfg["ds"]) for v in range(N)]
            if all(ok for ok, _ in checks):
                break
        else:
            raise AssertionError(f"case {name}: no seed gives inputs the reference's result is specified on")
        assert all(ok for ok, _ in checks)
        for _, facts in checks:
            for k, v in facts.items():
                shown[k] = shown.get(k, False) or v
        away = examine(clouds[T - 1], mats[T * N - 1], cfg["hw"], cfg["ds"])
        depth, rcs, gt = reference_maps(L, clouds, mats, cfg)
        if N > 1:
            assert not depth[T * N - 1].any() and not rcs[T * N - 1].any(), "the view facing away keeps a point"
        ridx = np.flatnonzero(depth)
        assert np.array_equal(ridx, np.flatnonzero(rcs)), "radar_rcs is occupied elsewhere than radar_depth"
        lidx = np.flatnonzero(gt)
        off = np.zeros(T + 1, np.int32)
        off[1:] = np.cumsum([len(c) for c in clouds])
        out.update({f"{name}:hw": np.array(cfg["hw"]), f"{name}:ds": np.array(cfg["ds"]), f"{name}:depth": np.array(DEPTH),
                    f"{name}:n_views": np.array(N), f"{name}:points": np.concatenate(clouds), f"{name}:offsets": off,
                    f"{name}:lidar2img": mats, f"{name}:radar_idx": ridx, f"{name}:radar_depth": depth.ravel()[ridx],
                    f"{name}:radar_rcs": rcs.ravel()[ridx], f"{name}:lidar_idx": lidx, f"{name}:lidar_depth": gt.ravel()[lidx]})
        hm, wm = cfg["hw"][0] // cfg["ds"], cfg["hw"][1] // cfg["ds"]
        print(f"case {name}: seed {seed}, {len(ridx) // hm} radar columns, {len(lidx)} lidar pixels, top rank {int(lidx.max() % (hm * wm)) if len(lidx) else 0}"
              f"{'' if away[0] else ' (!)'}")
    missing = [k for k, v in shown.items() if not v]
    assert not missing, f"the cases do not show: {missing}"
    assert any(k.endswith(":lidar_idx") and len(v) and (v % (256 * 704)).max() > (1 << 17) for k, v in out.items()), "no rank above 2^17"
    np.savez_compressed(os.path.join(HERE, "point_maps_small.npz"), **out)
    print("shown:", shown)


if __name__ == "__main__":
    main()
