"""racformer_amd/image_aug.py on the CPU against the reference's own runs (tests/golden/image_aug_small.npz, written by
tests/golden/gen_golden_image_aug.py): values, the number and order of numpy draws, and that the caller's image stays.

Tolerance of the float64 comparison: both sides do the same float64 operations in the same order, so they agree to rounding;
1e-9 of the tensor's scale leaves room for a library that sums or divides in another order and is a million times below what any
wrong step of the chain would give."""
import os

import numpy as np
import pytest
import torch

from racformer_amd import image_aug as A

NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "image_aug_small.npz"))


def close(got, want):
    return float((got - want).abs().max()) <= 1e-9 * float(want.abs().max())


def test_photometric_distortion_matches_the_reference(golden):
    aug = A.GpuPhotoMetricDistortion()
    for s in golden["photo_seeds"]:
        x = torch.from_numpy(golden[f"photo:{s}:input"])
        keep = x.clone()
        np.random.seed(int(s))
        out = aug(x.double())
        assert np.random.rand() == float(golden[f"photo:{s}:next_rand"]), "another number of draws than the reference's"
        assert out.dtype == torch.float64 and close(out, torch.from_numpy(golden[f"photo:{s}:out64"]))
        np.random.seed(int(s))
        out32 = aug(x)
        assert torch.equal(x, keep), "the caller's image was modified"
        # float32: the same operations again, so the reference's float32 run up to the rounding of single steps
        want32 = torch.from_numpy(golden[f"photo:{s}:out32"])
        assert out32.dtype == torch.float32 and float((out32 - want32).abs().max()) <= 2.0 ** -20 * float(want32.abs().max())


def test_draw_then_apply_is_the_call(golden):
    s = int(golden["photo_seeds"][0])
    x = torch.from_numpy(golden[f"photo:{s}:input"]).double()
    aug = A.GpuPhotoMetricDistortion()
    np.random.seed(s)
    draws = aug.draw(x.shape[0])
    assert np.random.rand() == float(golden[f"photo:{s}:next_rand"])
    assert len(draws) == x.shape[0] and {d.mode for d in draws} <= {0, 1}
    assert close(aug.apply(x, draws), torch.from_numpy(golden[f"photo:{s}:out64"]))
    with pytest.raises(ValueError):
        aug.apply(x, draws[:-1])


def test_constructor_arguments_are_the_references():
    aug = A.GpuPhotoMetricDistortion(brightness_delta=8, contrast_range=(0.9, 1.1), saturation_range=(0.8, 1.2), hue_delta=4)
    assert (aug.brightness_delta, aug.contrast_lower, aug.contrast_upper, aug.saturation_lower, aug.saturation_upper, aug.hue_delta) \
        == (8, 0.9, 1.1, 0.8, 1.2, 4)
    d = A.GpuPhotoMetricDistortion()
    assert (d.brightness_delta, d.contrast_lower, d.contrast_upper, d.saturation_lower, d.saturation_upper, d.hue_delta) \
        == (32, 0.5, 1.5, 0.5, 1.5, 18)
    g = A.GridMask()
    assert (g.ratio, g.prob) == (0.5, 0.7) and len(g.state_dict()) == 0 and not list(g.parameters()) and not list(g.buffers())


def test_grid_mask_matches_the_reference(golden):
    seen = set()
    for h, w, s in golden["grid_cases"]:
        key = f"grid:{h}x{w}:{s}"
        x = torch.from_numpy(golden[key + ":input"])
        keep = x.clone()
        m = A.GridMask(ratio=0.5, prob=0.7).train()
        np.random.seed(int(s))
        out = m(x.double())
        assert np.random.rand() == float(golden[key + ":next_rand"])
        assert torch.equal(out, torch.from_numpy(golden[key + ":out64"]))
        np.random.seed(int(s))
        out32 = m(x)
        assert torch.equal(out32, torch.from_numpy(golden[key + ":out32"])) and torch.equal(x, keep)
        applied = int(golden[key + ":applied"])
        assert (out32 is x) == (not applied)
        seen.add(((int(h), int(w)), applied))
    assert len(seen) == 4           # applied and skipped at both sizes


def test_grid_mask_returns_its_input_in_eval_and_above_prob():
    x = torch.rand(2, 3, 16, 48)
    m = A.GridMask().eval()
    np.random.seed(0)               # (rand() = 0.549 <= prob: only eval() keeps the mask off)
    assert m(x) is x
    a = np.random.rand()
    np.random.seed(0)
    np.random.rand()
    assert np.random.rand() == a, "eval() draws rand() once, as the reference's short-circuit does"
    m.train()
    np.random.seed(4)               # (rand() = 0.967 > prob)
    assert m(x) is x
    np.random.seed(0)
    assert m(x) is not x
    np.random.seed(0)
    assert A.GridMask(prob=0.5).train()(x) is x


def test_grid_mask_keeps_the_bands():
    """The reference's ``1 - mask``: the bands of width l every d pixels stay, everything else is zeroed."""
    d = A.GridDraw(d=6, l=3, st_h=1, st_w=4)
    m = A.GridMask.mask(d, 16, 48)
    hh, ww = 24, 72
    full = np.zeros((hh, ww), np.uint8)
    for i in range(hh // 6):
        full[6 * i + 1:6 * i + 4, :] = 1
    for i in range(ww // 6):
        full[:, 6 * i + 4:6 * i + 7] = 1
    assert np.array_equal(m, full[4:20, 12:60])


@pytest.mark.parametrize("shape,div", [((2, 16, 44), None), ((3, 23, 37), 16)])
def test_identity_parameters_normalise_and_pad(shape, div):
    n, H, W = shape
    x = torch.rand(n, 3, H, W, dtype=torch.float64) * 255
    keep = x.clone()
    out = A.prepare_images(x, None, NORM, div, None)
    Hp, Wp = A.padded_size(H, W, div)
    mean = torch.tensor(NORM["mean"], dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor(NORM["std"], dtype=torch.float64).view(1, 3, 1, 1)
    want = torch.zeros(n, 3, Hp, Wp, dtype=torch.float64)
    want[:, :, :H, :W] = (x[:, [2, 1, 0]] - mean) / std
    assert out.shape == want.shape and torch.equal(out, want) and torch.equal(x, keep)
    assert (Hp, Wp) == ((H, W) if div is None else (32, 48))


def test_prepare_composes_the_four_steps(golden):
    """prepare_images_torch = colour, normalise, pad, mask -- in this order (the reference pads the NORMALISED image and masks the padded one)."""
    s = int(golden["photo_seeds"][1])
    x = torch.from_numpy(golden[f"photo:{s}:input"]).double()[:, :, :15, :43]
    aug, gm = A.GpuPhotoMetricDistortion(), A.GridMask().train()
    np.random.seed(s)
    photo = aug.draw(x.shape[0])
    np.random.seed(0)
    grid = gm.draw(16)
    assert grid is not None
    out = A.prepare_images_torch(x, photo, NORM, 16, grid)
    step = aug.apply(x, photo)[:, [2, 1, 0]]
    step = (step - torch.tensor(NORM["mean"], dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(NORM["std"], dtype=torch.float64).view(1, 3, 1, 1)
    step = torch.nn.functional.pad(step, [0, 5, 0, 1])
    mask = torch.from_numpy(A.GridMask.mask(grid, 16, 48)).double()
    assert torch.equal(out, step * mask)
    assert out.shape[-2:] == (16, 48) and float(out[:, :, 15:].abs().max()) == 0 and float(out[:, :, :, 43:].abs().max()) == 0


def test_parameter_table_folds_the_channel_maps():
    """Output channel k = working RGB channel map[k]: checked against the torch route on an image whose channels are constants."""
    x = torch.zeros(1, 3, 2, 2, dtype=torch.float64)
    x[0, 0], x[0, 1], x[0, 2] = 10.0, 20.0, 30.0          # B, G, R
    for perm in ([0, 1, 2], [1, 2, 0], [2, 0, 1], [0, 2, 1]):
        dr = [A.PhotoDraw(0, None, None, None, None, perm)]
        for to_rgb in (True, False):
            cfg = dict(mean=[0, 0, 0], std=[1, 1, 1], to_rgb=to_rgb)
            out = A.prepare_images_torch(x, dr, cfg, None, None)
            tab = A.parameter_table(1, dr, to_rgb)
            rgb = [30.0, 20.0, 10.0]
            # (round: the HSV round trip with its eps = 1e-8 returns 20.000001 for 20)
            assert [round(float(out[0, k, 0, 0]), 3) for k in range(3)] == [rgb[int(tab[0, 6 + k])] for k in range(3)]
    assert A.parameter_table(2, None, True)[:, 0].tolist() == [0.0, 0.0]
