"""rac_image_aug_fwd (csrc/image_aug.hip) on the device against the float64 torch route of racformer_amd/image_aug.py (pinned to
the reference by tests/test_image_aug_cpu.py) on the same drawn parameters.

Rule (that of tests/test_depth_net_gpu.py, RATIO imported from there): max |kernel - float64| <= RATIO x E_ref + one float32 ulp at
the tensor's scale, E_ref = the float32 torch route's own error against float64 on the same case (CPU).  The composite map is
continuous -- at channel ties, grey pixels and sector boundaries either branch gives the same value -- so no pixel is exempt.
Masked pixels and pad pixels are exactly 0.0.

Shapes (n, H, W, size_divisor):
  golden   6 x 16 x 44, none   the fixture's images (integer-valued, quantised with ties, grey and black columns) under the fixture's
                               seeds; W and Wp multiples of 4: the 16-byte path, no pad
  one      1 x 16 x 44, none   a single image
  odd      7 x 23 x 37, 16     -> 32 x 48: W odd, the scalar path, pad rows and pad columns, a group that straddles the image's edge
  vecpad   2 x 12 x 40, 16     -> 16 x 48: the 16-byte path with pad rows and whole pad groups
Every case runs with colour + mask, and with identity parameters (no colour, no mask)."""
import os

import numpy as np
import pytest
import torch

from racformer_amd import image_aug as A
from test_depth_net_gpu import RATIO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
CASES = {"golden3": (6, 16, 44, None), "golden11": (6, 16, 44, None), "one": (1, 16, 44, None), "odd": (7, 23, 37, 16),
         "vecpad": (2, 12, 40, 16)}
GRID_SEED = 0            # np.random.seed(0): rand() = 0.549 <= 0.7, the mask applies
_REF = {}


def case(name, golden_dir):
    """Input, draws, float64 reference and E_ref of one case, with and without augmentation: computed once, shared, not modified."""
    if name in _REF:
        return _REF[name]
    n, H, W, div = CASES[name]
    if name.startswith("golden"):
        seed = int(name[6:])
        x = torch.from_numpy(np.load(os.path.join(golden_dir, "image_aug_small.npz"))[f"photo:{seed}:input"])
    else:
        seed = 40 + sorted(CASES).index(name)
        x = torch.from_numpy(np.random.RandomState(seed).uniform(0, 255, size=(n, 3, H, W)).astype(np.float32))
    assert tuple(x.shape) == (n, 3, H, W)
    np.random.seed(seed)
    photo = A.GpuPhotoMetricDistortion().draw(n)
    Hp, Wp = A.padded_size(H, W, div)
    np.random.seed(GRID_SEED)
    grid = A.GridMask().train().draw(Hp)
    assert grid is not None
    out = {}
    for kind, (p, g) in dict(aug=(photo, grid), identity=(None, None)).items():
        r64 = A.prepare_images_torch(x.double(), p, NORM, div, g)
        r32 = A.prepare_images_torch(x, p, NORM, div, g)
        out[kind] = dict(photo=p, grid=g, r64=r64, e_ref=float((r32.double() - r64).abs().max()))
    _REF[name] = dict(x=x, div=div, Hp=Hp, Wp=Wp, **out)
    return _REF[name]


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("kind", ["aug", "identity"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_against_float64(name, kind, golden_dir):
    c = case(name, golden_dir)
    k = c[kind]
    x = c["x"].to(DEV)
    keep = x.clone()
    got = A.prepare_images(x, k["photo"], NORM, c["div"], k["grid"])
    again = A.prepare_images(x, k["photo"], NORM, c["div"], k["grid"])
    torch.cuda.synchronize()
    r64 = k["r64"]
    assert got.shape == r64.shape and got.dtype == torch.float32 and got.is_contiguous()
    err = float((got.double().cpu() - r64).abs().max())
    tol = RATIO * k["e_ref"] + 2.0 ** -23 * float(r64.abs().max())
    print(f"{name}:{kind}: E_ref {k['e_ref']:.3g}, kernel {err:.3g} (allowed {tol:.3g}), scale {float(r64.abs().max()):.3g}")
    assert err <= tol
    assert torch.equal(bits(got), bits(again)), "two runs differ"
    assert torch.equal(bits(x), bits(keep)), "the input was modified"
    n, _, H, W = c["x"].shape
    g = got.cpu()
    assert float(g[:, :, H:].abs().max() if c["Hp"] > H else 0.0) == 0.0 and float(g[:, :, :, W:].abs().max() if c["Wp"] > W else 0.0) == 0.0
    if k["grid"] is not None:
        mask = torch.from_numpy(A.GridMask.mask(k["grid"], c["Hp"], c["Wp"])).bool()
        assert (~mask).any() and mask.any()
        assert float(g[:, :, ~mask].abs().max()) == 0.0, "a masked pixel is not exactly 0"
        assert torch.equal(g[:, :, ~mask], torch.zeros_like(g[:, :, ~mask]))


def test_colour_without_mask_and_mask_without_colour(golden_dir):
    c = case("odd", golden_dir)
    x = c["x"].to(DEV)
    for photo, grid in ((c["aug"]["photo"], None), (None, c["aug"]["grid"])):
        r64 = A.prepare_images_torch(c["x"].double(), photo, NORM, c["div"], grid)
        e_ref = float((A.prepare_images_torch(c["x"], photo, NORM, c["div"], grid).double() - r64).abs().max())
        got = A.prepare_images(x, photo, NORM, c["div"], grid)
        assert float((got.double().cpu() - r64).abs().max()) <= RATIO * e_ref + 2.0 ** -23 * float(r64.abs().max())


def test_without_norm_and_without_to_rgb(golden_dir):
    c = case("vecpad", golden_dir)
    x = c["x"].to(DEV)
    for cfg in (None, dict(NORM, to_rgb=False)):
        r64 = A.prepare_images_torch(c["x"].double(), c["aug"]["photo"], cfg, c["div"], c["aug"]["grid"])
        e_ref = float((A.prepare_images_torch(c["x"], c["aug"]["photo"], cfg, c["div"], c["aug"]["grid"]).double() - r64).abs().max())
        got = A.prepare_images(x, c["aug"]["photo"], cfg, c["div"], c["aug"]["grid"])
        assert float((got.double().cpu() - r64).abs().max()) <= RATIO * e_ref + 2.0 ** -23 * float(r64.abs().max())


def test_non_contiguous_and_misaligned_inputs(golden_dir):
    c = case("golden3", golden_dir)
    k = c["aug"]
    want = A.prepare_images(c["x"].to(DEV), k["photo"], NORM, None, k["grid"])
    # a channel-last view of the same values: made contiguous inside
    nc = c["x"].to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not nc.is_contiguous()
    assert torch.equal(bits(A.prepare_images(nc, k["photo"], NORM, None, k["grid"])), bits(want))
    # a contiguous image that starts 4 bytes into its storage: the scalar path, the same bits
    flat = torch.empty(c["x"].numel() + 1, device=DEV)
    off = flat[1:].view(c["x"].shape)
    off.copy_(c["x"])
    assert off.data_ptr() % 16 != 0
    assert torch.equal(bits(A.prepare_images(off, k["photo"], NORM, None, k["grid"])), bits(want))


def test_what_the_hip_route_refuses(golden_dir):
    c = case("one", golden_dir)
    x = c["x"].to(DEV)
    with pytest.raises(ValueError):
        A.image_aug_fwd(x.double())
    with pytest.raises(ValueError):
        A.image_aug_fwd(x[:, :2])
    with pytest.raises(ValueError):
        A.image_aug_fwd(x, photo=[])
    with pytest.raises(RuntimeError, match="grid mask"):
        A.image_aug_fwd(x, grid=A.GridDraw(4, 4, 0, 0))
    # float64 on the device takes the torch route
    out = A.prepare_images(x.double(), None, NORM, None, None)
    assert out.dtype == torch.float64 and out.is_cuda
