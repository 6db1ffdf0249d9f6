"""The image augmentations the reference "moved to the GPU" for a training step -- ``GpuPhotoMetricDistortion`` (models/utils.py
:219-305) and ``GridMask`` (:8-45) -- and, around them, the whole image preparation of ``extract_feat`` (models/racformer.py
:198-224, :108-109): colour distortion, the ``img_norm_cfg`` step, zero padding up to ``size_divisor``, grid mask.

Draws.  The reference draws from numpy's global generator; a seeded run here makes exactly its calls in its order.  ``draw`` of
either class does the drawing and returns a small record, ``apply`` / ``forward`` work from a record, so the same drawn parameters
can be given to both routes.  Nothing is drawn differently on the device than on the CPU.

Two routes:
  torch   ``GpuPhotoMetricDistortion.apply``, ``GridMask.apply``, ``prepare_images_torch``: the reference's tensor operations step by
          step (quirks included: no clipping, the single hue wrap, ``x * mask``) on any device in any floating dtype, float64
          included.  The oracle of the other route.
  HIP     ``prepare_images`` on device float32 tensors: ONE launch (``rac_image_aug_fwd``, csrc/image_aug.hip) reads the raw image
          once and writes once the normalised, padded, masked image the stem takes as it is.  The per-image parameters travel as one
          small host table copied once per call; every channel shuffle (BGR -> RGB, the random permutation, RGB -> BGR, ``to_rgb``)
          is folded into one channel map; the grid mask is computed from its four integers, no mask tensor is built.  Identity
          parameters -- no colour record, no mask record -- are valid: the launch then normalises and pads only.

The caller's image is never modified (the reference's in-place operations act on a fancy-indexed copy, too)."""
import ctypes
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from numpy import random

from . import _lib
from .resnet import norm_args

TABLE_COLS = 9      # csrc/image_aug.hip: colour, delta, alpha0, sat, hue, alpha1, map[3]

# One image's drawn distortion: each value is None where its coin came up 0 (the reference then skips the operation).
PhotoDraw = namedtuple("PhotoDraw", "mode delta alpha sat hue perm")
# The four integers of an applied grid mask (l derived from d as the reference does).
GridDraw = namedtuple("GridDraw", "d l st_h st_w")


# ------------------------------------------------------------------------------------------------------------ colour conversions
def rgb_to_hsv(image, eps=1e-8):
    """models/utils.py:123-175 (an image in 0..255 -> h in degrees, s, v in 0..255)."""
    image = image / 255.0
    max_rgb, argmax_rgb = image.max(-3)
    min_rgb, _ = image.min(-3)
    deltac = max_rgb - min_rgb
    v = max_rgb
    s = deltac / (max_rgb + eps)
    deltac = torch.where(deltac == 0, torch.ones_like(deltac), deltac)
    rc, gc, bc = torch.unbind((max_rgb.unsqueeze(-3) - image), dim=-3)
    h1 = bc - gc
    h2 = (rc - bc) + 2.0 * deltac
    h3 = (gc - rc) + 4.0 * deltac
    h = torch.stack((h1, h2, h3), dim=-3) / deltac.unsqueeze(-3)
    h = torch.gather(h, dim=-3, index=argmax_rgb.unsqueeze(-3)).squeeze(-3)
    h = (h / 6.0) % 1.0
    h = h * 360.0
    v = v * 255.0
    return torch.stack((h, s, v), dim=-3)


def hsv_to_rgb(image):
    """models/utils.py:178-216."""
    h = image[..., 0, :, :] / 360.0
    s = image[..., 1, :, :]
    v = image[..., 2, :, :] / 255.0
    hi = torch.floor(h * 6) % 6
    f = ((h * 6) % 6) - hi
    one = torch.tensor(1.0, device=image.device, dtype=image.dtype)
    p = v * (one - s)
    q = v * (one - f * s)
    t = v * (one - (one - f) * s)
    hi = hi.long()
    indices = torch.stack([hi, hi + 6, hi + 12], dim=-3)
    out = torch.stack((v, q, p, p, t, v, t, v, v, q, p, p, p, p, t, v, v, q), dim=-3)
    out = torch.gather(out, -3, indices)
    return out * 255.0


# ------------------------------------------------------------------------------------------------------------ the two classes
class GpuPhotoMetricDistortion:
    """The reference's class (:219-305): constructor arguments, defaults and the order of its numpy draws."""

    def __init__(self, brightness_delta=32, contrast_range=(0.5, 1.5), saturation_range=(0.5, 1.5), hue_delta=18):
        self.brightness_delta = brightness_delta
        self.contrast_lower, self.contrast_upper = contrast_range
        self.saturation_lower, self.saturation_upper = saturation_range
        self.hue_delta = hue_delta

    def draw(self, n):
        """The reference's calls of numpy's global generator for ``n`` images, in its order -> a list of n ``PhotoDraw``."""
        modes = [random.randint(2) for _ in range(n)]
        delta, alpha, sat, hue, perm = [None] * n, [None] * n, [None] * n, [None] * n, [None] * n
        for i in range(n):
            if random.randint(2):
                delta[i] = random.uniform(-self.brightness_delta, self.brightness_delta)
            if modes[i] == 0:
                if random.randint(2):
                    alpha[i] = random.uniform(self.contrast_lower, self.contrast_upper)
        for i in range(n):
            if random.randint(2):
                sat[i] = random.uniform(self.saturation_lower, self.saturation_upper)
            if random.randint(2):
                hue[i] = random.uniform(-self.hue_delta, self.hue_delta)
        for i in range(n):
            if modes[i] == 1:
                if random.randint(2):
                    alpha[i] = random.uniform(self.contrast_lower, self.contrast_upper)
            if random.randint(2):
                perm[i] = [int(k) for k in random.permutation(3)]
        return [PhotoDraw(int(modes[i]), delta[i], alpha[i], sat[i], hue[i], perm[i]) for i in range(n)]

    @staticmethod
    def apply(imgs, draws):
        """imgs [n, 3, H, W] (BGR, 0..255, any floating dtype) with the drawn parameters, step by step as :255-305."""
        if len(draws) != imgs.shape[0]:
            raise ValueError(f"GpuPhotoMetricDistortion: {len(draws)} draws for {imgs.shape[0]} images")
        imgs = imgs[:, [2, 1, 0], :, :]  # BGR to RGB (a copy: the caller's image stays)
        for idx, dr in enumerate(draws):
            if dr.delta is not None:
                imgs[idx] += dr.delta
            if dr.mode == 0 and dr.alpha is not None:
                imgs[idx] *= dr.alpha
        imgs = rgb_to_hsv(imgs)
        for idx, dr in enumerate(draws):
            if dr.sat is not None:
                imgs[idx, 1] *= dr.sat
            if dr.hue is not None:
                imgs[idx, 0] += dr.hue
        imgs[:, 0][imgs[:, 0] > 360] -= 360
        imgs[:, 0][imgs[:, 0] < 0] += 360
        imgs = hsv_to_rgb(imgs)
        for idx, dr in enumerate(draws):
            if dr.mode == 1 and dr.alpha is not None:
                imgs[idx] *= dr.alpha
            if dr.perm is not None:
                imgs[idx] = imgs[idx, dr.perm]
        return imgs[:, [2, 1, 0], :, :]  # RGB to BGR

    def __call__(self, imgs):
        return self.apply(imgs, self.draw(imgs.shape[0]))


class GridMask(nn.Module):
    """The reference's module (:8-45); no parameters or buffers.  One draw serves all images of a call."""

    def __init__(self, ratio=0.5, prob=0.7):
        super().__init__()
        self.ratio = ratio
        self.prob = prob

    def draw(self, h):
        """``np.random.rand()`` always; ``randint(2, h)``, ``randint(d)``, ``randint(d)`` only where the mask applies (``h``: the
        height of the image the mask is laid over, the padded one in the detector) -> ``GridDraw`` or None."""
        if np.random.rand() > self.prob or not self.training:
            return None
        d = np.random.randint(2, h)
        l = min(max(int(d * self.ratio + 0.5), 1), d - 1)
        st_h = np.random.randint(d)
        st_w = np.random.randint(d)
        return GridDraw(int(d), int(l), int(st_h), int(st_w))

    @staticmethod
    def mask(draw, h, w):
        """The uint8 numpy mask [h, w] AFTER the reference's ``1 - mask``: 1 on the bands, 0 elsewhere (:20-41)."""
        hh, ww = int(1.5 * h), int(1.5 * w)
        d, l = draw.d, draw.l
        mask = np.ones((hh, ww), np.uint8)
        for i in range(hh // d):
            s = d * i + draw.st_h
            t = min(s + l, hh)
            mask[s:t, :] = 0
        for i in range(ww // d):
            s = d * i + draw.st_w
            t = min(s + l, ww)
            mask[:, s:t] = 0
        mask = mask[(hh - h) // 2:(hh - h) // 2 + h, (ww - w) // 2:(ww - w) // 2 + w]
        return 1 - mask

    @classmethod
    def apply(cls, x, draw):
        if draw is None:
            return x
        n, c, h, w = x.size()
        mask = torch.tensor(cls.mask(draw, h, w), dtype=x.dtype, device=x.device)
        return (x.reshape(-1, h, w) * mask.expand(n * c, h, w)).view(n, c, h, w)

    def forward(self, x):
        return self.apply(x, self.draw(x.shape[2]))


# ------------------------------------------------------------------------------------------------------------ the preparation
def padded_size(H, W, size_divisor):
    if not size_divisor:
        return H, W
    return -(-H // size_divisor) * size_divisor, -(-W // size_divisor) * size_divisor


def prepare_images_torch(img, photo=None, norm_cfg=None, size_divisor=None, grid=None):
    """img [n, 3, H, W] -> [n, 3, Hp, Wp], the reference's steps in the image's dtype: ``GpuPhotoMetricDistortion.apply`` (``photo``:
    the n draws, or None), the img_norm_cfg step (``norm_cfg``: the dict with mean / std / to_rgb, or None), zero padding of the
    normalised image at the bottom and right, ``GridMask.apply`` (``grid``: a ``GridDraw`` or None)."""
    if photo is not None:
        img = GpuPhotoMetricDistortion.apply(img, photo)
    if norm_cfg is not None:
        perm, mean, std = norm_args(norm_cfg)
        if perm != [0, 1, 2]:
            img = img[:, perm, :, :]
        img = img - torch.tensor(mean, device=img.device, dtype=img.dtype).reshape(1, 3, 1, 1)
        img = img / torch.tensor(std, device=img.device, dtype=img.dtype).reshape(1, 3, 1, 1)
    H, W = img.shape[-2:]
    Hp, Wp = padded_size(H, W, size_divisor)
    if (Hp, Wp) != (H, W):
        img = F.pad(img, [0, Wp - W, 0, Hp - H], value=0)
    return GridMask.apply(img, grid)


def parameter_table(n, photo=None, to_rgb=False):
    """The kernel's per-image table, float64 numpy [n, 9]: colour flag, delta, alpha0, sat, hue, alpha1 and the channel map -- output
    channel k takes the working channel (R, G, B = 0, 1, 2) ``map[k]``.  After the permutation ``new[k] = rgb[perm[k]]`` the
    reference flips to BGR, and ``to_rgb`` flips back: with ``to_rgb`` the map is the permutation, without it its reverse."""
    tab = np.zeros((n, TABLE_COLS), np.float64)
    tab[:, 2] = tab[:, 3] = tab[:, 5] = 1.0
    for i in range(n):
        perm = [0, 1, 2]
        if photo is not None:
            dr = photo[i]
            tab[i, 0] = 1.0
            tab[i, 1] = 0.0 if dr.delta is None else dr.delta
            if dr.alpha is not None:
                tab[i, 2 if dr.mode == 0 else 5] = dr.alpha
            tab[i, 3] = 1.0 if dr.sat is None else dr.sat
            tab[i, 4] = 0.0 if dr.hue is None else dr.hue
            if dr.perm is not None:
                perm = list(dr.perm)
        tab[i, 6:9] = perm if to_rgb else perm[::-1]
    return tab


def device_table(n, photo, norm_cfg, device):
    """``parameter_table`` as the float32 device tensor the kernel reads: one small host tensor, copied once."""
    to_rgb = norm_cfg is not None and norm_args(norm_cfg)[0] != [0, 1, 2]
    return torch.from_numpy(parameter_table(n, photo, to_rgb).astype(np.float32)).to(device)


def image_aug_fwd(img, photo=None, norm_cfg=None, size_divisor=None, grid=None, table=None):
    """The HIP route alone: img float32 device [n, 3, H, W] -> [n, 3, Hp, Wp] in one ``rac_image_aug_fwd`` launch.  A non-contiguous
    image is made contiguous first.  ``table``: ``device_table(n, photo, norm_cfg, device)`` built beforehand (then ``photo`` is not
    looked at); by default it is built and copied here."""
    if img.dim() != 4 or img.shape[1] != 3 or img.dtype != torch.float32:
        raise ValueError(f"image_aug_fwd: a float32 [n, 3, H, W] image expected, got {img.dtype} {tuple(img.shape)}")
    if photo is not None and len(photo) != img.shape[0]:
        raise ValueError(f"image_aug_fwd: {len(photo)} draws for {img.shape[0]} images")
    img = img.detach().contiguous()
    _lib.require_gpu(img, what="image_aug_fwd")
    n, _, H, W = img.shape
    Hp, Wp = padded_size(H, W, size_divisor)
    mean, std = None, None
    if norm_cfg is not None:
        _, m, s = norm_args(norm_cfg)
        mean, std = (ctypes.c_float * 3)(*m), (ctypes.c_float * 3)(*s)      # (host arrays: read before the launch returns)
    if table is None:
        table = device_table(n, photo, norm_cfg, img.device)
    elif tuple(table.shape) != (n, TABLE_COLS) or table.dtype != torch.float32 or table.device != img.device or not table.is_contiguous():
        raise ValueError(f"image_aug_fwd: a contiguous float32 [{n}, {TABLE_COLS}] table on the image's device expected")
    out = torch.empty(n, 3, Hp, Wp, dtype=torch.float32, device=img.device)
    g = grid if grid is not None else GridDraw(0, 0, 0, 0)
    host = lambda a: ctypes.cast(a, ctypes.c_void_p) if a is not None else None         # noqa: E731
    rc = _lib.lib().rac_image_aug_fwd(_lib.ptr(img), _lib.ptr(table), _lib.ptr(out), n, H, W, Hp, Wp, host(mean), host(std), g.d, g.l, g.st_h, g.st_w,
                                      _lib.stream_ptr())
    _lib.check(rc, "rac_image_aug_fwd")
    return out


def prepare_images(img, photo=None, norm_cfg=None, size_divisor=None, grid=None):
    """The image preparation of a training step on given draws: the HIP launch on device float32 tensors, the torch route elsewhere."""
    if img.is_cuda and img.dtype == torch.float32:
        return image_aug_fwd(img, photo, norm_cfg, size_divisor, grid)
    return prepare_images_torch(img, photo, norm_cfg, size_divisor, grid)
