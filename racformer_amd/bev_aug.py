"""The BEV augmentation of the reference's data pipeline, ``RaCGlobalRotScaleTransImage`` (loaders/pipelines/transforms.py:398-464): one
random rotation about z and one isotropic scaling of the whole scene -- every ``lidar2img``, the lidar cloud, the T radar clouds and the
ground-truth boxes -- and the two annotation filters that stand in front of it in the recipe (``ObjectRangeFilter``,
``ObjectNameFilter``), all on plain tensors: no mmdet3d object is needed.

Draws.  ``RaCGlobalRotScaleTransImage.draw`` makes the reference's two calls of numpy's global generator in its order and returns a
``BevDraw``; everything else works from such a record.  ``view_mats`` makes the new ``lidar2img`` by the reference's own torch calls
(float32 ``cos`` / ``sin`` of the angle, ``torch.inverse`` of the 4 x 4, ``M.float() @ rot_inv`` and then ``@ scale_inv``).

The rule.  The reference's clouds and boxes go through mmdet3d's ``rotate`` / ``scale``, a library matmul whose
summation order nobody specifies, so the order is fixed here.  ``draw_row`` gives a draw's four float32 numbers: ``a`` the angle,
``c = cos(a)`` and ``s = sin(a)`` by torch on the CPU, ``r`` the ratio.  Every operation is rounded once, nothing is contracted:
  point row  [x, y, z, ...]:  x' = ((x c + y (-s)) + z 0) r,  y' = ((x s + y c) + z 0) r,  z' = ((x 0 + y 0) + z 1) r; columns >= 3
             are copied bit for bit -- the radar rows' velocity columns 4 and 5 included, which ``BasePoints.rotate`` leaves alone.  The
             products by 0 stay: they spread a NaN or inf coordinate over the row as the matmul does.
  box row    [x, y, z, w, l, h, yaw, vx, vy] (bottom centre):  the centre as a point; w, l, h times r; yaw' = yaw + a, not re-limited;
             vx' = (vx c + vy (-s)) r, vy' = (vx s + vy c) r.  Seven-column boxes carry no velocity.
NaN payloads are not part of the rule (which operand's payload an addition of two NaNs keeps is the hardware's choice).

Two routes:
  torch   ``bev_aug_torch``: the rule elementwise, in the stated order, on any device and in float32 or float64.  The oracle of the
          other route; ``__call__`` (the reference's dict behaviour on the host: rotate everything, then scale everything) is made of
          the same steps, so it gives the same bits.
  HIP     ``BevAugPlan`` on device tensors: ONE launch (``rac_bev_aug_fwd``, csrc/bev_aug.hip) for all clouds and box sets of all
          samples.  The host makes a segment table (source, destination, rows, columns, kind, sample) and a chunk table (256 rows of
          one segment each; the grid), uploaded in one copy and good for as long as the tensors stay; the draws travel in a small
          float table ``[B, 4]`` the launch reads, so a captured launch takes new draws from a rewritten table.
``transform_batch`` is what ``RaCFormer.prepare_bev_aug`` calls: the clouds of a batch into the ``pack_clouds`` layout, either route."""
import ctypes
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib

CHUNK, MAX_COLS = _lib.BEV_CHUNK, _lib.BEV_MAX_COLS
POINTS, BOXES = _lib.BEV_POINTS, _lib.BEV_BOXES
KINDS = {"points": POINTS, "boxes": BOXES}
# rac_bev_seg / rac_bev_chunk (include/racformer_hip.h)
_SEG = np.dtype([("src", "<u8"), ("dst", "<u8"), ("rows", "<i4"), ("cols", "<i4"), ("kind", "<i4"), ("sample", "<i4")])
_CHUNK = np.dtype([("seg", "<i4"), ("row0", "<i4")])

# One sample's drawn transformation: the angle about z (radians) and the scale ratio, as numpy's generator returned them.
BevDraw = namedtuple("BevDraw", "rot_angle scale_ratio")


# ------------------------------------------------------------------------------------------------------------ matrices and scalars
def _rot_inv(angle):
    """``rotate_z``'s inverse matrix (:428-438): the angle as a float32 tensor, its float32 cos and sin, ``torch.inverse``."""
    rot_cos = torch.cos(torch.tensor(float(angle)))
    rot_sin = torch.sin(torch.tensor(float(angle)))
    rot_mat = torch.tensor([[rot_cos, -rot_sin, 0, 0], [rot_sin, rot_cos, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    return torch.inverse(rot_mat)


def _scale_inv(ratio):
    """``scale_xyz``'s inverse matrix (:449-456)."""
    ratio = float(ratio)
    return torch.inverse(torch.tensor([[ratio, 0, 0, 0], [0, ratio, 0, 0], [0, 0, ratio, 0], [0, 0, 0, 1]]))


def _mat_step(mats, inv):
    return [(torch.tensor(np.asarray(m)).float() @ inv).numpy() for m in mats]


def view_mats(lidar2img, draw):
    """The new ``lidar2img`` of a draw, by the reference's calls in its order and dtypes: a list of float32 [4, 4] arrays."""
    return _mat_step(_mat_step(lidar2img, _rot_inv(draw.rot_angle)), _scale_inv(draw.scale_ratio))


def draw_row(draw):
    """(c, s, a, r) of a draw as float32 numpy [4]: the angle rounded to float32 as ``tensor.new_tensor(angle)`` rounds it, its cos
    and sin by torch on the CPU (the very values ``view_mats`` uses), the ratio rounded to float32."""
    a = torch.tensor(float(draw.rot_angle))
    return np.array([float(torch.cos(a)), float(torch.sin(a)), float(a), float(torch.tensor(float(draw.scale_ratio)))], np.float32)


def draw_table(draws, device=None):
    """The kernel's float32 table [B, 4] of B draws.  One small host tensor, copied once."""
    table = torch.from_numpy(np.stack([draw_row(d) for d in draws]))
    return table if device is None else table.to(device)


def _scalars(t, row):
    """The row's four numbers as 0-dim tensors of ``t``'s dtype on its device (made from host numbers: nothing is read back)."""
    return [torch.tensor(float(v), dtype=t.dtype, device=t.device) for v in np.asarray(row, np.float32)]


# ------------------------------------------------------------------------------------------------------------ the rule in torch
def _rot_xyz(t, c, s):
    x, y, z = t[:, 0], t[:, 1], t[:, 2]
    zero, one = torch.zeros_like(c), torch.ones_like(c)
    xc, ys, xs, yc, z0 = x * c, y * (-s), x * s, y * c, z * zero        # (every product a tensor of its own: nothing can fuse)
    x0, y0, z1 = x * zero, y * zero, z * one
    return (xc + ys) + z0, (xs + yc) + z0, (x0 + y0) + z1


def _check(t, kind):
    if t.dim() != 2 or not t.is_floating_point() or (t.shape[1] < 3 if kind == POINTS else t.shape[1] not in (7, 9)):
        raise ValueError(f"bev_aug: a floating [n, {'>= 3' if kind == POINTS else '7 or 9'}] tensor expected, got {t.dtype} {tuple(t.shape)}")


def rotate_rows(t, kind, row):
    """The rotation step alone (``rotate(angle)`` of the reference's objects) -> a new tensor."""
    _check(t, kind)
    c, s, a, _ = _scalars(t, row)
    out = t.clone()
    out[:, 0], out[:, 1], out[:, 2] = _rot_xyz(t, c, s)
    if kind == BOXES:
        out[:, 6] = t[:, 6] + a
        if t.shape[1] == 9:
            vx, vy = t[:, 7], t[:, 8]
            vxc, vys, vxs, vyc = vx * c, vy * (-s), vx * s, vy * c
            out[:, 7], out[:, 8] = vxc + vys, vxs + vyc
    return out


def scale_rows(t, kind, row):
    """The scaling step alone (``scale(ratio)``) -> a new tensor."""
    _check(t, kind)
    r = _scalars(t, row)[3]
    out = t.clone()
    upto = 3 if kind == POINTS else 6
    out[:, :upto] = t[:, :upto] * r
    if kind == BOXES and t.shape[1] == 9:
        out[:, 7:9] = t[:, 7:9] * r
    return out


def bev_aug_torch(t, row, kind="points"):
    """The rule on one cloud (``kind='points'``) or box set (``'boxes'``) ``t`` [n, C] with ``row`` = ``draw_row(draw)`` -> a new
    tensor of ``t``'s dtype on its device: the rotation step, then the scaling step, each operation rounded once."""
    kind = KINDS[kind] if isinstance(kind, str) else kind
    return scale_rows(rotate_rows(t, kind, row), kind, row)


# ------------------------------------------------------------------------------------------------------------ the class
def _tensor_of(obj):
    return obj if isinstance(obj, torch.Tensor) else obj.tensor


def _replace(container, key, new):
    """Puts the transformed rows where the old ones were: a plain tensor is replaced, an object with ``.tensor`` keeps its identity."""
    if isinstance(container[key], torch.Tensor):
        container[key] = new
    else:
        container[key].tensor = new


# the steps ``__call__`` is made of, by the names of the reference's method calls (argument: the angle / the ratio as drawn)
def rotate_points(t, angle):
    return rotate_rows(t, POINTS, draw_row(BevDraw(angle, 1.0)))


def rotate_boxes(t, angle):
    return rotate_rows(t, BOXES, draw_row(BevDraw(angle, 1.0)))


def scale_points(t, ratio):
    return scale_rows(t, POINTS, draw_row(BevDraw(0.0, ratio)))


def scale_boxes(t, ratio):
    return scale_rows(t, BOXES, draw_row(BevDraw(0.0, ratio)))


BOX_KEYS = ("gt_bboxes_3d", "gt_bboxes_static3d", "gt_bboxes_dynamic3d")


class RaCGlobalRotScaleTransImage:
    """The reference's class (:398-464): its constructor, the order of its numpy draws, its dict behaviour."""

    def __init__(self, rot_range=[-0.3925, 0.3925], scale_ratio_range=[0.95, 1.05], translation_std=[0, 0, 0]):
        self.rot_range = rot_range
        self.scale_ratio_range = scale_ratio_range
        self.translation_std = translation_std          # (unused there as well: ":424 TODO: support translation")

    def draw(self):
        """The two draws of ``__call__`` (:409, :417) in their order -> ``BevDraw``.  (The reference makes the second one after it has
        rotated; nothing in between draws, so both can be made first.)"""
        rot_angle = np.random.uniform(*self.rot_range)
        scale_ratio = np.random.uniform(*self.scale_ratio_range)
        return BevDraw(rot_angle, scale_ratio)

    def _step(self, results, inv, points_fn, boxes_fn, value):
        for view in range(len(results['lidar2img'])):
            results['lidar2img'][view] = _mat_step([results['lidar2img'][view]], inv)[0]
        if 'points' in results:
            _replace(results, 'points', points_fn(_tensor_of(results['points']), value))
        if 'radar_points' in results:
            for i in range(len(results['radar_points'])):
                _replace(results['radar_points'], i, points_fn(_tensor_of(results['radar_points'][i]), value))
        for key in BOX_KEYS:
            if key in results:
                _replace(results, key, boxes_fn(_tensor_of(results[key]), value))

    def __call__(self, results, draw=None):
        """:407-426 on the host with plain tensors: everything is rotated, then everything is scaled, key by key in the reference's
        order (``lidar2img``, ``points``, ``radar_points[i]``, then the box keys).  ``draw``: a record made beforehand (by default one
        is drawn here).  Clouds and boxes are [n, C] tensors or objects with ``.tensor``; a missing optional key is skipped."""
        draw = self.draw() if draw is None else draw
        self._step(results, _rot_inv(draw.rot_angle), rotate_points, rotate_boxes, draw.rot_angle)
        self._step(results, _scale_inv(draw.scale_ratio), scale_points, scale_boxes, draw.scale_ratio)
        return results


# ------------------------------------------------------------------------------------------------------------ the annotation filters
class ObjectRangeFilter:
    """mmdet3d's ``ObjectRangeFilter`` on plain tensors: boxes whose centre lies strictly inside the BEV range
    (``x > lo_x & y > lo_y & x < hi_x & y < hi_y``) are kept, in input order, and their yaw is brought into [-pi, pi)
    (``limit_yaw(offset=0.5, period=2 pi)``: ``yaw - floor(yaw / 2 pi + 0.5) 2 pi``)."""

    def __init__(self, point_cloud_range):
        self.pcd_range = np.array(point_cloud_range, dtype=np.float32)

    def __call__(self, gt_bboxes_3d, gt_labels_3d):
        """(boxes [n, >= 7], labels [n], a tensor or an array) -> (boxes [m, ...], labels [m]); the inputs stay as they are."""
        box = gt_bboxes_3d
        lo_x, lo_y, _, hi_x, hi_y, _ = (float(v) for v in self.pcd_range)
        mask = (box[:, 0] > lo_x) & (box[:, 1] > lo_y) & (box[:, 0] < hi_x) & (box[:, 1] < hi_y)
        box = box[mask].clone()
        period = 2 * math.pi
        box[:, 6] = box[:, 6] - torch.floor(box[:, 6] / period + 0.5) * period
        labels = gt_labels_3d[mask] if isinstance(gt_labels_3d, torch.Tensor) else np.asarray(gt_labels_3d)[mask.numpy()]
        return box, labels


class ObjectNameFilter:
    """mmdet3d's ``ObjectNameFilter`` on plain tensors: a box is kept when its label indexes a name of ``class_names`` (by default
    ``classes`` itself) that is in ``classes``; labels outside ``class_names`` (-1: a category the dataset does not map) are dropped.
    Input order is kept."""

    def __init__(self, classes, class_names=None):
        self.classes = list(classes)
        self.class_names = self.classes if class_names is None else list(class_names)
        self.labels = [i for i, n in enumerate(self.class_names) if n in self.classes]

    def __call__(self, gt_bboxes_3d, gt_labels_3d):
        keep = np.isin(np.asarray(gt_labels_3d), self.labels)
        mask = torch.from_numpy(keep)
        labels = gt_labels_3d[mask] if isinstance(gt_labels_3d, torch.Tensor) else np.asarray(gt_labels_3d)[keep]
        return gt_bboxes_3d[mask], labels


# ------------------------------------------------------------------------------------------------------------ the HIP route
class BevAugPlan:
    """The device tables of one set of segments.  ``segments``: a list of ``(src, dst, kind, sample)`` -- contiguous float32 device
    tensors [n, C] of one shape each (``dst`` may be ``src`` itself), ``kind`` ``'points'`` / ``'boxes'``, ``sample`` the row of the
    draws table the segment uses.  Building uploads both tables in one copy; ``launch(draws)`` enqueues ``rac_bev_aug_fwd`` on the
    current stream and allocates, copies and reads back nothing, so it can be captured.  The plan holds its tensors: it is good for
    as long as they are the ones to transform."""

    def __init__(self, segments, n_samples):
        if not segments:
            raise ValueError("BevAugPlan: no segments")
        self.n_samples, self.tensors = int(n_samples), [(s, d) for s, d, _, _ in segments]
        dev = segments[0][0].device
        seg = np.zeros(len(segments), _SEG)
        chunks = []
        for i, (src, dst, kind, sample) in enumerate(segments):
            kind = KINDS[kind] if isinstance(kind, str) else kind
            _lib.require_gpu(src, dst, what="BevAugPlan")
            for t in (src, dst):
                _check(t, kind)
                if t.dtype != torch.float32 or t.device != dev:
                    raise ValueError(f"BevAugPlan: segment {i}: float32 tensors on one device expected, got {t.dtype} on {t.device}")
            if src.shape != dst.shape or src.shape[1] > MAX_COLS:
                raise ValueError(f"BevAugPlan: segment {i}: source {tuple(src.shape)} and destination {tuple(dst.shape)} (one shape, at "
                                 f"most {MAX_COLS} columns)")
            if not 0 <= sample < self.n_samples:
                raise ValueError(f"BevAugPlan: segment {i}: sample {sample} outside [0, {self.n_samples})")
            seg[i] = (src.data_ptr(), dst.data_ptr(), src.shape[0], src.shape[1], kind, sample)
            c = np.zeros(-(-src.shape[0] // CHUNK), _CHUNK)
            c["seg"], c["row0"] = i, np.arange(len(c)) * CHUNK
            chunks.append(c)
        chunks = np.concatenate(chunks)
        self.n_segs, self.n_chunks = len(seg), len(chunks)
        self.host = np.concatenate([seg.view(np.uint8), chunks.view(np.uint8), np.zeros(8, np.uint8)])     # (never empty: 0 chunks)
        self.device = torch.from_numpy(self.host).to(dev)
        self._chunk_at = seg.nbytes

    def launch(self, draws):
        """``draws``: the float32 device table [n_samples, 4] of ``draw_table``."""
        if draws.dtype != torch.float32 or tuple(draws.shape) != (self.n_samples, 4) or draws.device != self.device.device or \
                not draws.is_contiguous():
            raise ValueError(f"BevAugPlan.launch: a contiguous float32 [{self.n_samples}, 4] draws table on the segments' device expected")
        host = self.host.ctypes.data
        rc = _lib.lib().rac_bev_aug_fwd(_lib.ptr(self.device), ctypes.c_void_p(self.device.data_ptr() + self._chunk_at), ctypes.c_void_p(host),
                                        ctypes.c_void_p(host + self._chunk_at), _lib.ptr(draws), self.n_segs, self.n_chunks, self.n_samples,
                                        _lib.stream_ptr())
        _lib.check(rc, "rac_bev_aug_fwd")


def _offsets(counts):
    off = np.zeros(len(counts) + 1, np.int64)
    off[1:] = np.cumsum(counts)
    return off.tolist()


def transform_batch(radar_points, points, boxes, draws):
    """A batch through the rule.  ``radar_points``: a list over T of lists over B of [n, C] float32 clouds; ``points``: a list over B
    of lidar clouds, or None; ``boxes``: a list over B of [n, 7 or 9] box sets of one width, or None; ``draws``: B ``BevDraw``.
    -> (radar_points in the same nesting, points, boxes): views into three packed tensors in the ``pack_clouds`` layout (the radar
    clouds sample-major, ``[b][t]``, as ``RaCFormer.point_maps`` packs them).  Device tensors: one ``rac_bev_aug_fwd`` launch, which
    does the packing too; CPU tensors: ``bev_aug_torch`` per cloud."""
    B, T = len(draws), len(radar_points)
    if any(len(frame) != B for frame in radar_points) or (points is not None and len(points) != B) or (boxes is not None and len(boxes) != B):
        raise ValueError(f"bev_aug.transform_batch: {B} draws, but the clouds or boxes are not for {B} samples")
    groups = [([radar_points[t][b] for b in range(B) for t in range(T)], [b for b in range(B) for _ in range(T)], POINTS)]
    if points is not None:
        groups.append((list(points), list(range(B)), POINTS))
    if boxes is not None:
        groups.append((list(boxes), list(range(B)), BOXES))
    like = next((t for srcs, _, _ in groups for t in srcs), None)
    on_device = like is not None and like.is_cuda
    rows = [draw_row(d) for d in draws]
    views, segments = [], []
    for srcs, samples, kind in groups:
        if not srcs:
            views.append([])
            continue
        srcs = [s.detach().to(like.device) for s in srcs]          # (boxes the loader left on the host follow the clouds: a small upload)
        if any(s.dim() != 2 or s.shape[1] != srcs[0].shape[1] or s.dtype != torch.float32 for s in srcs):
            raise ValueError("bev_aug.transform_batch: the clouds (the box sets) have to be float32 [n, C] tensors of one width")
        off = _offsets([s.shape[0] for s in srcs])
        if on_device:
            packed = torch.empty(off[-1], srcs[0].shape[1], dtype=torch.float32, device=like.device)
            segments += [(s.contiguous(), packed[off[i]:off[i + 1]], kind, b) for i, (s, b) in enumerate(zip(srcs, samples))]
        else:
            packed = torch.cat([bev_aug_torch(s, rows[b], kind) for s, b in zip(srcs, samples)])
        views.append([packed[off[i]:off[i + 1]] for i in range(len(srcs))])
    if on_device and segments:
        BevAugPlan(segments, B).launch(draw_table(draws, like.device))
    radar = [[views[0][b * T + t] for b in range(B)] for t in range(T)]
    rest = iter(views[1:])
    return radar, (next(rest) if points is not None else None), (next(rest) if boxes is not None else None)
