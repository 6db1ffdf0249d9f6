#!/usr/bin/env python3
"""Golden vectors of the BEV augmentation: runs the REFERENCE's own ``RaCGlobalRotScaleTransImage.__call__``
(loaders/pipelines/transforms.py:398-464) on CPU and writes a data-only fixture next to this script.
Run in the build container only (needs the reference tree):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_bev_aug.py

``transforms.py`` is loaded by path under stub modules for what it imports at module level and never touches on this path (mmcv,
mmdet.datasets.builder).  The clouds and boxes of the results are recording stubs: mmdet3d is not there, and what the fixture pins is
what the reference's own code does -- the draws, the matrices, and which object gets which call with which argument in which order.

  bev_aug_small.npz, per case ``name`` (keys ``name:...``), under ``np.random.seed(seed)``:
      seed, rot_range [2], scale_ratio_range [2], draws [2] float64 (the angle, the ratio: the arguments the stubs received, asserted
      equal to the generator's next two ``uniform`` values after the seed),
      lidar2img_in [8, 4, 4] float64 (4 views x 2 frames), lidar2img_out [8, 4, 4] in the dtype the reference leaves (float32),
      log_key / log_op (strings), log_val float64, log_axis int64 (-1: not given), log_type (the argument's Python type name): one
      entry per ``rotate(angle, axis)`` / ``scale(ratio)`` call in call order; keys are ``points``, ``radar_points[i]``, ``gt_bboxes_3d``,
      ``gt_bboxes_static3d``, ``gt_bboxes_dynamic3d``.
  cases: a every optional cloud key, 2 radar clouds; b no ``points`` key, 3 radar clouds; c the static and dynamic box keys, no
  ``radar_points`` key, other ranges."""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("RACFORMER_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True

CASES = {
    "a": dict(seed=0, kwargs={}, points=True, radar=2, split=False),
    "b": dict(seed=1, kwargs={}, points=False, radar=3, split=False),
    "c": dict(seed=2, kwargs=dict(rot_range=[-0.7, 0.2], scale_ratio_range=[0.9, 1.2]), points=True, radar=None, split=True),
}


def load_transforms():
    class Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("mmcv")
    mod("mmdet")
    mod("mmdet.datasets")
    mod("mmdet.datasets.builder", PIPELINES=Registry())
    spec = importlib.util.spec_from_file_location("rac_reference_transforms", os.path.join(REF_ROOT, "loaders", "pipelines", "transforms.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


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


class Recorder:
    """Stands where a ``LiDARPoints`` / ``LiDARInstance3DBoxes`` would: notes every call."""

    def __init__(self, key, log):
        self.key, self.log = key, log

    def rotate(self, angle, axis=None):
        self.log.append((self.key, "rotate", float(np.asarray(angle)), -1 if axis is None else int(axis), type(angle).__name__))

    def scale(self, ratio):
        self.log.append((self.key, "scale", float(ratio), -1, type(ratio).__name__))


def main():
    T = load_transforms()
    out = {}
    for name, cfg in CASES.items():
        t = T.RaCGlobalRotScaleTransImage(**cfg["kwargs"])
        mats = np.stack([camera((256, 704), 2 * np.pi * v / 4 + 0.03 * f, (0.4 + 0.1 * v, 0.2 * f, 1.5 + 0.01 * v)) for f in range(2)
                         for v in range(4)])
        log = []
        results = dict(lidar2img=[m.copy() for m in mats], gt_bboxes_3d=Recorder("gt_bboxes_3d", log))
        if cfg["points"]:
            results["points"] = Recorder("points", log)
        if cfg["radar"] is not None:
            results["radar_points"] = [Recorder(f"radar_points[{i}]", log) for i in range(cfg["radar"])]
        if cfg["split"]:
            results["gt_bboxes_static3d"] = Recorder("gt_bboxes_static3d", log)
            results["gt_bboxes_dynamic3d"] = Recorder("gt_bboxes_dynamic3d", log)
        np.random.seed(cfg["seed"])
        t(results)
        np.random.seed(cfg["seed"])
        draws = np.array([np.random.uniform(*t.rot_range), np.random.uniform(*t.scale_ratio_range)])
        rot = [e[2] for e in log if e[1] == "rotate"]
        sca = [e[2] for e in log if e[1] == "scale"]
        assert rot and sca and all(v == draws[0] for v in rot) and all(v == draws[1] for v in sca), "the draws are not the generator's next two"
        new = np.stack(results["lidar2img"])
        assert new.shape == (8, 4, 4)
        out.update({f"{name}:seed": np.array(cfg["seed"]), f"{name}:rot_range": np.array(t.rot_range, np.float64),
                    f"{name}:scale_ratio_range": np.array(t.scale_ratio_range, np.float64), f"{name}:draws": draws,
                    f"{name}:lidar2img_in": mats, f"{name}:lidar2img_out": new,
                    f"{name}:log_key": np.array([e[0] for e in log]), f"{name}:log_op": np.array([e[1] for e in log]),
                    f"{name}:log_val": np.array([e[2] for e in log], np.float64), f"{name}:log_axis": np.array([e[3] for e in log], np.int64),
                    f"{name}:log_type": np.array([e[4] for e in log])})
        print(f"case {name}: seed {cfg['seed']}, draws {draws.tolist()}, lidar2img {new.dtype}, {len(log)} calls: "
              + ", ".join(f"{e[0]}.{e[1]}" for e in log))
    np.savez_compressed(os.path.join(HERE, "bev_aug_small.npz"), **out)


if __name__ == "__main__":
    main()
