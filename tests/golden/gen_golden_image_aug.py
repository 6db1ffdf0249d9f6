#!/usr/bin/env python3
"""Golden vectors of the image augmentations: runs the REFERENCE's own ``GpuPhotoMetricDistortion`` and ``GridMask``
(models/utils.py:219-305, :8-45) on CPU under ``np.random.seed(s)`` and writes a data-only fixture next to this script.  Run in the
build container only (needs the reference tree, ``RACFORMER_REFERENCE`` or the default of ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_image_aug.py

models/utils.py needs only torch and numpy and is loaded on its own, by file path.

  image_aug_small.npz
    "photo_seeds", "grid_cases": the lists of cases
    per photometric case s ("photo:<s>:..."): six BGR images of 3 x 16 x 44 in 0..255 --
        image 0, 4, 5  uniform floats
        image 1        integer-valued
        image 2        quantised to multiples of 16, so that channels tie
        image 3        grey columns (three equal channels) and black columns among uniform ones
      input float32; out64 (the reference on input.double()) and out32 (on the float32 input); next_rand = one further
      np.random.rand() after the float64 call, which pins the number of draws (asserted equal after the float32 call).
    per GridMask case ("grid:<h>x<w>:<s>:..."): input float32 [2, 3, h, w], out64, out32, next_rand, applied (0 / 1); the module in
      training mode.
The generator asserts that the photometric seeds together show every coin in both states, both contrast modes, a permutation
that is not the identity, and a hue wrap on each side (h > 360 and h < 0 before the wrap); and that the GridMask seeds show both
"applied" and "skipped" at each size.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REF_ROOT = os.environ.get("RACFORMER_REFERENCE", "/root/reference")

PHOTO_SEEDS = (3, 11)
GRID_CASES = ((16, 48, 0), (16, 48, 4), (23, 37, 1), (23, 37, 4))      # (h, w, seed)
N, H, W = 6, 16, 44


def load_utils():
    spec = importlib.util.spec_from_file_location("rac_reference_models_utils", os.path.join(REF_ROOT, "models", "utils.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def photo_input(seed):
    rng = np.random.RandomState(1000 + seed)
    x = rng.uniform(0.0, 255.0, size=(N, 3, H, W))
    x[1] = np.floor(x[1])
    x[2] = np.floor(x[2] / 16.0) * 16.0
    x[3][:, :, 0:44:4] = x[3][0:1, :, 0:44:4]          # grey columns
    x[3][:, :, 1:44:8] = 0.0                           # black columns
    return torch.from_numpy(x.astype(np.float32))


class Spy:
    """Wraps numpy.random of the loaded module: the reference's own draws, recorded."""

    def __init__(self, real):
        self.real, self.coins, self.perms = real, [], []

    def randint(self, *a):
        v = self.real.randint(*a)
        self.coins.append(int(v))
        return v

    def uniform(self, *a):
        return self.real.uniform(*a)

    def permutation(self, n):
        p = self.real.permutation(n)
        self.perms.append([int(k) for k in p])
        return p


def main():
    R = load_utils()
    out = dict(photo_seeds=np.asarray(PHOTO_SEEDS), grid_cases=np.asarray(GRID_CASES))
    coins = {k: set() for k in ("brightness", "contrast0", "saturation", "hue", "contrast1", "swap")}
    perms, wraps_hi, wraps_lo, modes = [], 0, 0, set()
    real_rgb_to_hsv, real_hsv_to_rgb = R.rgb_to_hsv, R.hsv_to_rgb
    for s in PHOTO_SEEDS:
        x = photo_input(s)
        keep = x.clone()
        spy = Spy(R.random)
        seen = {}

        def hsv_to_rgb(image):
            seen["h"] = image[:, 0].clone()            # (after the wrap; the hue before it is h -+ 360 where it wrapped)
            return real_hsv_to_rgb(image)

        def rgb_to_hsv(image):
            res = real_rgb_to_hsv(image)
            seen["h0"] = res[:, 0].clone()
            return res

        R.random, R.rgb_to_hsv, R.hsv_to_rgb = spy, rgb_to_hsv, hsv_to_rgb
        try:
            np.random.seed(s)
            out64 = R.GpuPhotoMetricDistortion()(x.double())
            nxt = np.random.rand()
        finally:
            R.random, R.rgb_to_hsv, R.hsv_to_rgb = spy.real, real_rgb_to_hsv, real_hsv_to_rgb
        np.random.seed(s)
        out32 = R.GpuPhotoMetricDistortion()(x)
        assert np.random.rand() == nxt and torch.equal(x, keep)
        assert out32.dtype == torch.float32 and out64.dtype == torch.float64
        # a wrap shows as a hue that moved against its shift: shifted up past 360 it comes out below the unshifted hue, and the reverse
        moved = seen["h"] - seen["h0"]
        wraps_hi += int((moved < -300).sum())
        wraps_lo += int((moved > 300).sum())
        # the coins by kind, from the order of the reference's loops (:257-301)
        md, rest = spy.coins[:N], iter(spy.coins[N:])
        modes |= set(md)
        for i in range(N):
            coins["brightness"].add(next(rest))
            if md[i] == 0:
                coins["contrast0"].add(next(rest))
        for i in range(N):
            coins["saturation"].add(next(rest))
            coins["hue"].add(next(rest))
        for i in range(N):
            if md[i] == 1:
                coins["contrast1"].add(next(rest))
            coins["swap"].add(next(rest))
        assert next(rest, None) is None
        perms += spy.perms
        out[f"photo:{s}:input"] = x.numpy()
        out[f"photo:{s}:out64"] = out64.numpy()
        out[f"photo:{s}:out32"] = out32.numpy()
        out[f"photo:{s}:next_rand"] = np.float64(nxt)
        print(f"photo seed {s}: |out| <= {float(out64.abs().max()):.1f}, float32 against float64 {float((out32.double() - out64).abs().max()):.3g}")
    assert modes == {0, 1}, "both contrast modes"
    assert all(v == {0, 1} for v in coins.values()), f"every coin in both states: {coins}"
    assert any(p != [0, 1, 2] for p in perms), "a permutation that is not the identity"
    assert wraps_hi > 0 and wraps_lo > 0, f"a hue wrap on each side ({wraps_hi}, {wraps_lo})"

    applied = {}
    for h, w, s in GRID_CASES:
        rng = np.random.RandomState(2000 + s + h)
        x = torch.from_numpy(rng.uniform(-3.0, 3.0, size=(2, 3, h, w)).astype(np.float32))
        keep = x.clone()
        m = R.GridMask(ratio=0.5, prob=0.7).train()
        np.random.seed(s)
        out64 = m(x.double())
        nxt = np.random.rand()
        np.random.seed(s)
        out32 = m(x)
        assert np.random.rand() == nxt and torch.equal(x, keep)
        did = int(not torch.equal(out32, x))
        applied.setdefault((h, w), set()).add(did)
        for k, v in (("input", x.numpy()), ("out64", out64.numpy()), ("out32", out32.numpy()), ("next_rand", np.float64(nxt)), ("applied", np.int64(did))):
            out[f"grid:{h}x{w}:{s}:{k}"] = v
        print(f"grid {h}x{w} seed {s}: {'applied' if did else 'skipped'}, {int((out32 == 0).sum())} zeros")
    assert all(v == {0, 1} for v in applied.values()), f"applied and skipped at each size: {applied}"

    path = os.path.join(HERE, "image_aug_small.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
