"""The geometric image augmentation of the reference's data pipeline, ``RandomTransformImage`` (loaders/pipelines/transforms.py
:219-342): the raw camera frames (1600 x 900 in the f8 recipe) to the images ``extract_feat`` takes (704 x 256) -- Pillow's bicubic
``Image.resize``, ``crop``, the left-right flip -- with the same change folded into ``lidar2img``.

Draws.  ``RandomTransformImage.draw`` makes exactly the reference's calls of numpy's global generator in its order (the
``np.random.choice`` only where ``rand_flip`` is set, the ``uniform(*rot_lim)`` always) and returns an ``IdaDraw``; everything else
works from such a record, so one record serves both routes.  ``ida_mat`` is ``img_transform``'s matrix in its float32 torch operations.

Pixels.  Pillow resizes 8-bit images in fixed point: a horizontal pass and then a vertical pass, each rounded to uint8; the weights
of an output position are the bicubic filter (a = -0.5, support 2, stretched by the scale when down-scaling) sampled in float64,
normalised, and rounded to 22 fractional bits; a pass sums ``pixel * weight`` from 2^21 in an int32, shifts by 22 and clips to
0..255.  ``resample_coeffs`` is that table, ``resample_pass`` one pass, and the result equals Pillow's byte for byte.  The crop window
may leave the resized image on any side (Pillow fills with 0), the flip acts on the cropped window.  ``rotate != 0`` -- Pillow's
nearest-neighbour affine path, which none of the reference's configurations uses -- raises ``NotImplementedError`` on both routes.

Two routes:
  numpy   ``transform_images_numpy``: the passes above in integer arithmetic.  The oracle of the other route; ``__call__`` (the
          reference's dict behaviour on the host) takes its pixels from it and needs no Pillow.
  HIP     ``transform_images`` on a device uint8 tensor: ONE launch (``rac_image_geom_fwd``, csrc/image_geom.hip) for all images of all
          samples.  The host makes the coefficient tables of a sample's draw per OUTPUT column and row (the crop offset and the flip
          are folded into which resized column an output column reads; a position outside the resized image gets no taps, which
          sums to 0), pads them to the largest tap count and uploads them in one copy.  ``f32_chw`` writes the float32 [n, 3, fH, fW]
          image ``image_aug.prepare_images`` reads (values 0..255, the loader's channel order), ``u8_hwc`` the reference's own layout."""
import ctypes
from collections import namedtuple

import numpy as np
import torch

from . import _lib

PRECISION_BITS = 32 - 8 - 2         # Pillow's fixed point for 8-bit channels
TILE_W, TILE_H = 64, 16             # csrc/image_geom.hip: IG_TILE_W, IG_TILE_H
OUT_F32_CHW, OUT_U8_HWC = 0, 1
OUT_KINDS = {"f32_chw": OUT_F32_CHW, "u8_hwc": OUT_U8_HWC}

# One sample's drawn transformation, the tuple ``sample_augmentation`` returns: resize (a float), resize_dims (newW, newH), crop
# (left, upper, right, lower) in the resized image, flip, rotate (degrees).
IdaDraw = namedtuple("IdaDraw", "resize resize_dims crop flip rotate")


# ------------------------------------------------------------------------------------------------------------ Pillow's resampler
def bicubic_filter(x):
    """Pillow's bicubic kernel (a = -0.5) on a float64 array."""
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


def resample_weights(in_size, out_size):
    """``precompute_coeffs`` for the bicubic filter over the whole axis -> (bounds int32 [out, 2]: first tap and tap count, weights
    float64 [out, ksize], normalised, 0 past the count)."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(np.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    center = (np.arange(out_size) + 0.5) * scale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)                 # ((int): towards 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize)
    kk = np.where(x[None, :] < xmax[:, None], bicubic_filter((x[None, :] + xmin[:, None] - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(out_size)
    for t in range(ksize):          # (summed tap by tap, as the C loop does; a tap past the count adds +0.0)
        ww = ww + kk[:, t]
    kk = np.where(ww[:, None] != 0.0, kk / np.where(ww != 0.0, ww, 1.0)[:, None], kk)
    return np.stack([xmin, xmax], 1).astype(np.int32), kk


def resample_coeffs(in_size, out_size):
    """``precompute_coeffs`` + ``normalize_coeffs_8bpc`` -> (bounds int32 [out, 2], kk int32 [out, ksize]).  Asserts that an int32
    accumulator (Pillow's own type) cannot overflow in any order of summation."""
    bounds, w = resample_weights(in_size, out_size)
    kk = np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)).astype(np.int32)   # ((int): towards 0)
    assert np.all(255 * np.abs(kk.astype(np.int64)).sum(1) + (1 << (PRECISION_BITS - 1)) < (1 << 31)), \
        f"resample_coeffs({in_size}, {out_size}): an int32 accumulator could overflow"
    return bounds, kk


def identity_coeffs(size):
    """The table of a pass that is skipped: one tap of weight 1, which the fixed-point pass returns unchanged."""
    bounds = np.stack([np.arange(size), np.ones(size, np.int64)], 1).astype(np.int32)
    return bounds, np.full((size, 1), 1 << PRECISION_BITS, np.int32)


def resample_sums(img, bounds, kk, axis):
    """The unclipped int32 sums of one pass along ``axis`` of a uint8 array (2^21 included, not yet shifted)."""
    img = np.moveaxis(img, axis, 0)
    acc = np.full((len(bounds),) + img.shape[1:], 1 << (PRECISION_BITS - 1), np.int32)
    shape = (-1,) + (1,) * (img.ndim - 1)
    for t in range(kk.shape[1]):    # (a tap past the count has weight 0: its clamped index reads a pixel that does not matter)
        idx = np.minimum(bounds[:, 0] + t, img.shape[0] - 1)
        acc += img[idx].astype(np.int32) * kk[:, t].reshape(shape)
    return np.moveaxis(acc, 0, axis)


def resample_pass(img, bounds, kk, axis):
    """One pass of Pillow's 8-bit resampler along ``axis``: uint8 in, uint8 out."""
    return np.clip(resample_sums(img, bounds, kk, axis) >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize_numpy(img, new_w, new_h):
    """``Image.resize((new_w, new_h))`` (bicubic) of uint8 [..., H, W, C]: horizontal, then vertical; a pass whose size stays is skipped."""
    H, W = img.shape[-3:-1]
    if new_w != W:
        img = resample_pass(img, *resample_coeffs(W, new_w), axis=img.ndim - 2)
    if new_h != H:
        img = resample_pass(img, *resample_coeffs(H, new_h), axis=img.ndim - 3)
    return img


def final_dim(draw):
    """(fH, fW) of a draw's crop window."""
    return draw.crop[3] - draw.crop[1], draw.crop[2] - draw.crop[0]


def _no_rotation(draw, what):
    if draw.rotate != 0:
        raise NotImplementedError(f"{what}: rotate = {draw.rotate} (Pillow's nearest-neighbour rotation is not implemented; every "
                                  "configuration of the reference sets rot_lim = (0, 0))")


def transform_images_numpy(raw, draw):
    """raw uint8 [n, Hr, Wr, 3] -> uint8 [n, fH, fW, 3]: resize to ``draw.resize_dims``, the crop window (0 outside the resized
    image), the flip of the window."""
    _no_rotation(draw, "transform_images_numpy")
    raw = np.asarray(raw)
    if raw.dtype != np.uint8 or raw.ndim != 4:
        raise ValueError(f"transform_images_numpy: a uint8 [n, H, W, C] array expected, got {raw.dtype} {raw.shape}")
    new_w, new_h = draw.resize_dims
    img = resize_numpy(raw, new_w, new_h)
    left, upper, right, lower = draw.crop
    out = np.zeros((raw.shape[0], lower - upper, right - left, raw.shape[3]), np.uint8)
    x0, x1, y0, y1 = max(left, 0), min(right, new_w), max(upper, 0), min(lower, new_h)
    if x0 < x1 and y0 < y1:
        out[:, y0 - upper:y1 - upper, x0 - left:x1 - left] = img[:, y0:y1, x0:x1]
    if draw.flip:
        out = out[:, :, ::-1]
    return np.ascontiguousarray(out)


# ------------------------------------------------------------------------------------------------------------ the class
def ida_mat(draw):
    """``img_transform``'s 4 x 4 float32 matrix (:271-312): its float32 torch operations in its order, the rotation block included."""
    resize, _, crop, flip, rotate = draw
    ida_rot = torch.eye(2)
    ida_tran = torch.zeros(2)
    ida_rot *= resize
    ida_tran -= torch.Tensor(crop[:2])
    if flip:
        A = torch.Tensor([[-1, 0], [0, 1]])
        b = torch.Tensor([crop[2] - crop[0], 0])
        ida_rot = A.matmul(ida_rot)
        ida_tran = A.matmul(ida_tran) + b
    h = rotate / 180 * np.pi
    A = torch.Tensor([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])
    b = torch.Tensor([crop[2] - crop[0], crop[3] - crop[1]]) / 2
    b = A.matmul(-b) + b
    ida_rot = A.matmul(ida_rot)
    ida_tran = A.matmul(ida_tran) + b
    mat = torch.eye(4)
    mat[:2, :2] = ida_rot
    mat[:2, 2] = ida_tran
    return mat.numpy()


class RandomTransformImage:
    """The reference's class (:219-342): its constructor, the order of its numpy draws, its dict behaviour."""

    def __init__(self, ida_aug_conf=None, training=True):
        self.ida_aug_conf = ida_aug_conf
        self.training = training

    def draw(self):
        """``sample_augmentation`` (:314-342) -> ``IdaDraw``.  Nothing is drawn with ``training=False``."""
        conf = self.ida_aug_conf
        H, W = conf['H'], conf['W']
        fH, fW = conf['final_dim']
        if self.training:
            resize = np.random.uniform(*conf['resize_lim'])
            resize_dims = (int(W * resize), int(H * resize))
            newW, newH = resize_dims
            crop_h = int((1 - np.random.uniform(*conf['bot_pct_lim'])) * newH) - fH
            crop_w = int(np.random.uniform(0, max(0, newW - fW)))
            crop = (crop_w, crop_h, crop_w + fW, crop_h + fH)
            flip = False
            if conf['rand_flip'] and np.random.choice([0, 1]):
                flip = True
            rotate = np.random.uniform(*conf['rot_lim'])
        else:
            resize = max(fH / H, fW / W)
            resize_dims = (int(W * resize), int(H * resize))
            newW, newH = resize_dims
            crop_h = int((1 - np.mean(conf['bot_pct_lim'])) * newH) - fH
            crop_w = int(max(0, newW - fW) / 2)
            crop = (crop_w, crop_h, crop_w + fW, crop_h + fH)
            flip = False
            rotate = 0
        return IdaDraw(resize, resize_dims, crop, flip, rotate)

    def __call__(self, results, draw=None):
        """:225-269 on the host.  ``draw``: a record made beforehand (by default one is drawn here, as the reference does)."""
        draw = self.draw() if draw is None else draw
        n = len(results['img'])
        if len(results['lidar2img']) != n and n != 6:
            raise ValueError()
        mat = ida_mat(draw)
        for i in range(n):
            results['img'][i] = transform_images_numpy(np.uint8(results['img'][i])[None], draw)[0]
        for i in range(len(results['lidar2img'])):      # (one draw per call: every image's matrix is the same)
            results['lidar2img'][i] = mat @ results['lidar2img'][i]
        results['ori_shape'] = [img.shape for img in results['img']]
        results['img_shape'] = [img.shape for img in results['img']]
        results['pad_shape'] = [img.shape for img in results['img']]
        return results


# ------------------------------------------------------------------------------------------------------------ the HIP route
def _output_axis_table(in_size, new_size, start, out_size, flip):
    """The coefficient rows of one axis per OUTPUT position: output o reads resized position ``start + o`` (``start + out_size - 1 -
    o`` when flipped); outside [0, new_size) it gets no taps."""
    bounds, kk = resample_coeffs(in_size, new_size) if new_size != in_size else identity_coeffs(in_size)
    pos = start + (np.arange(out_size)[::-1] if flip else np.arange(out_size))
    inside = (pos >= 0) & (pos < new_size)
    at = np.clip(pos, 0, new_size - 1)
    b = np.where(inside[:, None], bounds[at], 0).astype(np.int32)
    k = np.where(inside[:, None], kk[at], 0).astype(np.int32)
    return b, k[:, :max(int(b[:, 1].max()), 1)]


def _tile_spans(bounds, tile):
    """Per tile of ``tile`` output positions: [first input position, one past the last] over its positions that have taps (0, 0 for none)."""
    n = -(-len(bounds) // tile)
    spans = np.zeros((n, 2), np.int32)
    for i in range(n):
        b = bounds[i * tile:(i + 1) * tile]
        b = b[b[:, 1] > 0]
        if len(b):
            spans[i] = b[:, 0].min(), (b[:, 0] + b[:, 1]).max()
    return spans


def geometry_tables(draws, raw_hw):
    """The kernel's tables for G draws, int32 numpy [G, words] and the tap count ``ksize`` they are padded to.  Per draw: column bounds
    [fW, 2], row bounds [fH, 2], the raw-column span of every tile column [ceil(fW / 64), 2], the raw-row span of every tile row
    [ceil(fH / 16), 2], column weights [fW, ksize], row weights [fH, ksize]."""
    Hr, Wr = raw_hw
    fH, fW = final_dim(draws[0])
    parts = []
    for d in draws:
        _no_rotation(d, "transform_images")
        if final_dim(d) != (fH, fW):
            raise ValueError(f"transform_images: the draws' crop windows differ in size: {final_dim(d)} and {(fH, fW)}")
        parts.append(_output_axis_table(Wr, d.resize_dims[0], d.crop[0], fW, d.flip) + _output_axis_table(Hr, d.resize_dims[1], d.crop[1], fH, False))
    ksize = max(max(hk.shape[1], vk.shape[1]) for _, hk, _, vk in parts)
    pad = lambda k: np.pad(k, [(0, 0), (0, ksize - k.shape[1])])       # noqa: E731
    rows = [np.concatenate([hb.ravel(), vb.ravel(), _tile_spans(hb, TILE_W).ravel(), _tile_spans(vb, TILE_H).ravel(), pad(hk).ravel(),
                            pad(vk).ravel()]) for hb, hk, vb, vk in parts]
    return np.ascontiguousarray(np.stack(rows).astype(np.int32)), ksize


GeomTables = namedtuple("GeomTables", "host device ksize")


def device_tables(draws, raw_hw, device):
    """``geometry_tables`` with its copy on the device (one small host array, copied once) -> ``GeomTables``."""
    host, ksize = geometry_tables(draws, raw_hw)
    return GeomTables(host, torch.from_numpy(host).to(device), ksize)


def image_geom_fwd(raw, draws, out="f32_chw", into=None, tables=None):
    """The HIP route alone: raw uint8 device [G * m, Hr, Wr, 3] and G draws -> one ``rac_image_geom_fwd`` launch.  ``into``: the output
    tensor to write (by default a new one).  ``tables``: ``device_tables(draws, (Hr, Wr), device)`` made beforehand; with both given
    the call allocates and copies nothing, so it can be captured into a graph."""
    if out not in OUT_KINDS:
        raise ValueError(f"transform_images: out = {out!r} (one of {sorted(OUT_KINDS)})")
    if raw.dim() != 4 or raw.shape[3] != 3 or raw.dtype != torch.uint8:
        raise ValueError(f"transform_images: a uint8 [n, H, W, 3] tensor expected, got {raw.dtype} {tuple(raw.shape)}")
    G = len(draws)
    if G == 0 or raw.shape[0] % G:
        raise ValueError(f"transform_images: {G} draws for {raw.shape[0]} images")
    _lib.require_gpu(raw, what="transform_images")
    n, Hr, Wr, _ = raw.shape
    fH, fW = final_dim(draws[0])
    if tables is None:
        tables = device_tables(draws, (Hr, Wr), raw.device)
    host, table, ksize = tables
    ntx, nty = -(-fW // TILE_W), -(-fH // TILE_H)
    words = 2 * (fW + fH + ntx + nty) + (fW + fH) * ksize
    if tuple(host.shape) != (G, words) or host.dtype != np.int32 or not host.flags.c_contiguous or tuple(table.shape) != (G, words) or \
            table.dtype != torch.int32 or table.device != raw.device or not table.is_contiguous():
        raise ValueError(f"transform_images: contiguous int32 [{G}, {words}] tables on the host and on the images' device expected")
    shape, dtype = ((n, 3, fH, fW), torch.float32) if out == "f32_chw" else ((n, fH, fW, 3), torch.uint8)
    if into is None:
        into = torch.empty(shape, dtype=dtype, device=raw.device)
    elif tuple(into.shape) != shape or into.dtype != dtype or into.device != raw.device or not into.is_contiguous():
        raise ValueError(f"transform_images: a contiguous {dtype} {shape} output on the images' device expected")
    rc = _lib.lib().rac_image_geom_fwd(_lib.ptr(raw), _lib.ptr(table), host.ctypes.data_as(ctypes.c_void_p), _lib.ptr(into), n, n // G, Hr, Wr,
                                       fH, fW, ksize, OUT_KINDS[out], _lib.stream_ptr())
    _lib.check(rc, "rac_image_geom_fwd")
    return into


def transform_images(raw, draws, out="f32_chw"):
    """raw uint8 [G * m, Hr, Wr, 3] with G draws, each for m consecutive images -> float32 [G * m, 3, fH, fW] (``f32_chw``) or uint8
    [G * m, fH, fW, 3] (``u8_hwc``): the HIP launch on device tensors, the numpy route on CPU tensors."""
    if raw.is_cuda:
        return image_geom_fwd(raw, draws, out)
    if out not in OUT_KINDS:
        raise ValueError(f"transform_images: out = {out!r} (one of {sorted(OUT_KINDS)})")
    G = len(draws)
    if G == 0 or raw.shape[0] % G:
        raise ValueError(f"transform_images: {G} draws for {raw.shape[0]} images")
    m = raw.shape[0] // G
    res = torch.from_numpy(np.concatenate([transform_images_numpy(raw[g * m:(g + 1) * m].numpy(), d) for g, d in enumerate(draws)]))
    return res.permute(0, 3, 1, 2).float().contiguous() if out == "f32_chw" else res
