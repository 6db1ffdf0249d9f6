"""The detector that joins the parts: ``RaCFormer`` of the reference's models/racformer.py -- images, radar clouds and the
radar depth / RCS maps (given, or made here from the radar clouds: ``radar_depth=None, radar_rcs=None``, racformer_amd/point_maps.py) to boxes, offline (``simple_test_offline``: all T frames of a sample through the front end) and streaming
(``simple_test_online``: only the frames the memory does not hold yet).

Constructor arguments are the ``model`` dict entries of configs/racformer_r50_nuimg_704x256_f8.py:108-201; every sub-config is a dict
(its ``type`` is checked and dropped) or an already built module.  Submodule names are the reference's, so a reference checkpoint loads
with ``strict=True``: ``img_backbone`` (``resnet.ResNet``), ``img_neck`` (``necks.FPN``), ``img_lss_neck`` (``necks.CustomFPN``; the very
``img_neck`` when ``num_lss_fpn == img_neck.num_outs``, :65-70), ``img_lss_view_transformer``
(``lss_depth.LSSViewTransformerBEVDepth_racformer``), ``radar_voxel_encoder`` / ``radar_bev_conv`` (the children of a
``radar_pillars.RadarPillarEncoder``, registered here directly; the encoder object itself stays out of the module tree, so no extra
prefix appears) and ``pts_bbox_head`` (``head.RaCFormer_head``, which gets ``train_cfg['pts']`` / ``test_cfg['pts']`` as the reference's
detector base hands them over).  ``data_aug['img_norm_cfg']`` becomes ``img_backbone.input_norm`` (the stem applies :202-212),
``data_aug['img_pad_cfg']`` is ``pad_multiple`` (models/utils.py:104-120; a no-op at multiples of the divisor).

Routing: on device tensors every part takes its HIP route; on CPU tensors its torch route, with the reference's layouts (the decoder
itself has no CPU route: ``pts_bbox_head`` raises there).  Departure, attribute ``pregrouped`` (default on): where the neck's
``hip_route`` holds, ``extract_feat`` returns the pyramid in the decoder's sampling layout -- per level ``[B*T*G, N, H, W, 64]`` from
``FPN.forward_pregrouped`` -- instead of ``[B, T*N, C, H, W]``, and sets ``pts_bbox_head.transformer.decoder.pregrouped`` to match what
it returned; the regroup copy then never runs.

Raw frames: ``prepare_raw`` takes what the cameras deliver -- uint8 frames and their metas -- through the loader's
``RandomTransformImage`` on the device (racformer_amd/image_geom.py: one launch for all frames of all samples) and returns the ``img``
and ``img_metas`` every entry point below takes as it is.  ``prepare_bev_aug`` is the loader's next geometric stage,
``RaCGlobalRotScaleTransImage`` (racformer_amd/bev_aug.py: the scene's rotation and scaling of all clouds and boxes in one launch).

Streaming (``simple_test_online``, :476-557, quirks included): batch size 1; a frame's key is its first camera's file name; a frame not
in the memory goes through ``extract_feat`` alone (T = 1, the metas of this call), so a cached BEV map stays in the ego frame of the
call that first saw it; a key repeated inside a window is computed once; after the call the oldest keys leave while the memory holds
16 or more.  The memory is one ring per tensor kind (four pyramid levels, the LSS BEV map, the radar BEV map) of ``15 + num_frames``
slots on the inputs' device, allocated once per shape; a new frame is copied into its slot.  The decoder's window -- T frames of
every kind, contiguous -- is assembled from the ring by ONE launch (``fused.frames_gather`` -> ``rac_frames_gather``) into buffers that
stay put; from the second call on these buffers are the ``inputs`` of a ``graph.CapturedStep`` (``capture``, default on), so a steady
step is: the front end on one frame, one slot copy per kind, one gather launch, ``CapturedStep.replay(img_metas)``.  On CPU tensors the
same bookkeeping runs with ``torch.index_select``.

Training (opt-in: ``det.fused_grad = True`` and ``det.train()``; off, ``forward(return_loss=True)``, ``forward_train`` and
``extract_feat`` in training mode raise ``TRAINING_MESSAGE`` as before).  Setting the switch sets ``fused_grad`` on ``img_backbone``,
``img_neck``, ``img_lss_neck`` and the radar encoder; ``AdaptiveMixing.fused_linear_grad`` stays the user's choice.
``extract_feat`` in training mode is :179-348 with ``stop_prev_grad == 0``: the images of all B*T*N views go through ONE launch
(``image_aug.prepare_images`` -> ``rac_image_aug_fwd``: ``color_aug`` where ``data_aug['img_color_aug']``, the img_norm_cfg step, the zero
padding, ``grid_mask`` while ``use_grid_mask``; numpy's global generator is drawn from exactly as the reference draws), the stem runs
with ``input_norm`` bypassed, backbone and necks run under autograd on the plain pyramid layout (``pregrouped`` is off for the call: the
decoder's regroup has a backward, ``forward_pregrouped`` has none); frame 0's radar branch and view transformer run in training mode
under autograd (batch statistics, running statistics updated once, ASPP's dropout live; the library's convolutions of DepthNet's torch
route on their deterministic algorithms, ``library_deterministic``, so that a seeded forward repeats bit for bit), frames 1 .. T-1 in
eval mode under ``no_grad`` on the statistics frame 0 has just updated.  Departure: only these two branches are toggled, where the reference calls ``self.eval()`` /
``self.train()`` on the whole detector and so un-freezes whatever the user had put into ``eval()``.  ``self.training and
stop_prev_grad > 0`` raises ``NotImplementedError``: the reference's branch calls the view transformer with three arguments and hands
all frames' clouds to ``extract_pts_feat`` -- it cannot run.  ``forward_train`` (:400-441, ``forward_pts_train`` :351-382) writes the
ground truth into the metas, runs the head in training mode and returns ``loss_depth`` plus the head's losses.  On CPU tensors every
part takes its torch route up to the decoder, which has none: the loss half is device-only, as inference is.  A training step empties
the streaming memory (its frames were computed on other weights); after ``train()`` or ``load_state_dict`` the next streaming call
compares the head's weights with those its captured plan was made on, once, and drops the plan if they differ (a steady streaming
step does not look at the weights; after editing weights in place in eval mode, call ``reset_memory()``).  ``with_cp`` is accepted and without effect.  The optimiser side of a step -- AdamW with the recipe's per-parameter learning rates, the gradient clip, the
schedule, ``train_step`` -- is ``racformer_amd/optim.py`` (its update moves every parameter's ``_version``, so no pack cached here goes stale); data-parallel training is not here."""
import contextlib
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F

from .bev_aug import RaCGlobalRotScaleTransImage, transform_batch, view_mats
from .head import RaCFormer_head
from .image_aug import GpuPhotoMetricDistortion, GridMask, prepare_images
from .image_geom import ida_mat, transform_images
from .lss_depth import LSSViewTransformerBEVDepth_racformer
from .necks import FPN, CustomFPN
from .point_maps import lidar_depth_map, meta_view_table, radar_maps
from .radar_pillars import RadarPillarEncoder, pack_clouds
from .resnet import ResNet, apply_input_norm

MEMORY_KEYS = 16        # the reference evicts while its queue holds this many keys (:551)
TRAINING_MESSAGE = ("racformer_amd.RaCFormer is built for inference unless its fused_grad switch is set: without it the radar branch "
                    "(RadarPillarEncoder) refuses training-mode BatchNorm, so forward(return_loss=True) / forward_train / extract_feat in "
                    "training mode are not implemented; set det.fused_grad = True (and det.train()) to opt in")


def _cfg(cfg, expected, what):
    """A sub-config dict without its ``type`` (which has to name ``expected``)."""
    cfg = dict(cfg)
    t = cfg.pop("type", expected)
    if t != expected:
        raise NotImplementedError(f"RaCFormer: {what} of type {t!r} is not implemented ({expected} expected)")
    return cfg


def pad_multiple(inputs, img_metas, size_divisor=32):
    """models/utils.py:104-120: zero padding at the bottom / right up to a multiple, the metas' shapes rewritten."""
    _, _, img_h, img_w = inputs.shape
    pad_h = 0 if img_h % size_divisor == 0 else size_divisor - (img_h % size_divisor)
    pad_w = 0 if img_w % size_divisor == 0 else size_divisor - (img_w % size_divisor)
    N = len(img_metas[0]['ori_shape'])
    for meta in img_metas:
        meta['img_shape'] = [(img_h + pad_h, img_w + pad_w, 3) for _ in range(N)]
        meta['pad_shape'] = [(img_h + pad_h, img_w + pad_w, 3) for _ in range(N)]
    if pad_h == 0 and pad_w == 0:
        return inputs
    return F.pad(inputs, [0, pad_w, 0, pad_h], value=0)


def bbox3d2result(bboxes, scores, labels):
    """mmdet3d.core.bbox3d2result: the three results on the host.  ``boxes_3d`` is the plain [k, 9] tensor of ``get_bboxes``."""
    return dict(boxes_3d=bboxes.to('cpu'), scores_3d=scores.cpu(), labels_3d=labels.cpu())


@contextlib.contextmanager
def library_deterministic(on=True):
    """The library's convolutions on their deterministic algorithms for the block (``torch.backends.cudnn.deterministic``, restored
    afterwards).  ``DepthNet`` in training mode takes its torch route, i.e. the library's convolutions, and by default those do not
    give the same bits twice on this device (measured: the first 3x3 convolution of ``reduce_conv`` already differs run to run; with
    the flag set every module's output repeats).  The training step wraps frame 0's forward in this, so that a seeded forward is
    reproducible; the backward runs outside it."""
    if not on:
        yield
        return
    was = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        yield
    finally:
        torch.backends.cudnn.deterministic = was


class FrameMemory:
    """The streaming route's store: per tensor kind one ring ``[n_slots, *frame]`` on the frames' device, keys in arrival order."""

    def __init__(self, n_slots, pregrouped):
        self.n_slots, self.pregrouped = n_slots, pregrouped
        self.rings = None
        self.slots = OrderedDict()          # key -> slot, oldest first
        self.free = list(range(n_slots - 1, -1, -1))

    def fits(self, tensors, n_slots, pregrouped):
        return self.rings is not None and n_slots <= self.n_slots and pregrouped == self.pregrouped and len(tensors) == len(self.rings) and all(
            r.shape[1:] == t.shape and r.device == t.device and r.dtype == t.dtype for r, t in zip(self.rings, tensors))

    def allocate(self, tensors):
        self.rings = [t.new_empty((self.n_slots,) + tuple(t.shape)) for t in tensors]

    def put(self, key, tensors):
        slot = self.free.pop()
        for ring, t in zip(self.rings, tensors):
            ring[slot].copy_(t)
        self.slots[key] = slot
        return slot

    def evict(self, limit=MEMORY_KEYS):
        while len(self.slots) >= limit:
            _, slot = self.slots.popitem(last=False)
            self.free.append(slot)


class RaCFormer(nn.Module):
    """models/racformer.py:18-557: inference, and the training step behind the ``fused_grad`` switch (module docstring)."""

    def __init__(self, data_aug=None, stop_prev_grad=False, pts_voxel_layer=None, pts_voxel_encoder=None, pts_middle_encoder=None,
                 pts_fusion_layer=None, img_backbone=None, pts_backbone=None, img_neck=None, num_lss_fpn=2, dep_downsample=16,
                 img_lss_neck=None, img_lss_view_transformer=None, pre_process=None, pts_neck=None, radar_voxel_layer=None,
                 radar_voxel_encoder=None, radar_middle_encoder=None, pts_bbox_head=None, img_roi_head=None, img_rpn_head=None,
                 train_cfg=None, test_cfg=None, pretrained=None, num_cams=6):
        super().__init__()
        if pre_process is not None:
            raise NotImplementedError("RaCFormer: pre_process (a backbone over the BEV map) is not used by the f8 configuration and not implemented")
        for name, given in (("pts_voxel_layer", pts_voxel_layer), ("pts_voxel_encoder", pts_voxel_encoder),
                            ("pts_middle_encoder", pts_middle_encoder), ("pts_fusion_layer", pts_fusion_layer),
                            ("pts_backbone", pts_backbone), ("pts_neck", pts_neck), ("img_roi_head", img_roi_head),
                            ("img_rpn_head", img_rpn_head)):
            if given is not None:
                raise NotImplementedError(f"RaCFormer: {name} is not used by the f8 configuration and not implemented")
        self.num_cams, self.data_aug, self.stop_prev_grad = num_cams, data_aug, stop_prev_grad
        self.dep_downsample, self.num_lss_fpn = dep_downsample, num_lss_fpn
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.pre_process = False
        self.pregrouped = True      # return the pyramid in the sampling layout where the neck's HIP route holds (module docstring)
        self.capture = True         # streaming on the device: replay a captured decoder step from the second call on
        # training: frame 0's forward with the library's convolutions on their deterministic algorithms (``library_deterministic``).  The
        # flag is process-wide while it is set: switch this off where other threads run library convolutions of their own, or where
        # the library's default algorithm matters more than a forward that repeats bit for bit
        self.deterministic_forward = True
        self.color_aug = GpuPhotoMetricDistortion()
        self.grid_mask = GridMask(ratio=0.5, prob=0.7)
        self.use_grid_mask = True

        self.img_backbone = img_backbone if isinstance(img_backbone, nn.Module) else ResNet(**_cfg(img_backbone, "ResNet", "img_backbone"))
        if data_aug is not None and 'img_norm_cfg' in data_aug:
            self.img_backbone.input_norm = data_aug['img_norm_cfg']
        if isinstance(img_neck, nn.Module):
            self.img_neck = img_neck
        else:
            ncfg = _cfg(img_neck, "FPN", "img_neck")
            ncfg.setdefault("num_cams", num_cams)
            self.img_neck = FPN(**ncfg)
        if img_lss_neck is not None:
            if self.num_lss_fpn == self.img_neck.num_outs:
                self.img_lss_neck = self.img_neck
            elif isinstance(img_lss_neck, nn.Module):
                self.img_lss_neck = img_lss_neck
            else:
                self.img_lss_neck = CustomFPN(**_cfg(img_lss_neck, "CustomFPN", "img_lss_neck"))
        else:
            self.img_lss_neck = None
        if isinstance(img_lss_view_transformer, nn.Module):
            self.img_lss_view_transformer = img_lss_view_transformer
        else:
            self.img_lss_view_transformer = LSSViewTransformerBEVDepth_racformer.from_config(
                **_cfg(img_lss_view_transformer, "LSSViewTransformerBEVDepth_racformer", "img_lss_view_transformer"))

        if isinstance(pts_bbox_head, nn.Module):
            self.pts_bbox_head = pts_bbox_head
        else:
            hcfg = _cfg(pts_bbox_head, "RaCFormer_head", "pts_bbox_head")
            if train_cfg and train_cfg.get("pts") is not None:
                hcfg["train_cfg"] = train_cfg["pts"]            # (with it the assigner: mmdet3d's MVXTwoStageDetector does the same)
            if test_cfg and test_cfg.get("pts") is not None:
                hcfg["test_cfg"] = test_cfg["pts"]
            self.pts_bbox_head = RaCFormer_head(**hcfg)

        if isinstance(radar_voxel_encoder, RadarPillarEncoder):
            enc = radar_voxel_encoder
        else:
            enc = RadarPillarEncoder({k: v for k, v in dict(radar_voxel_layer).items() if k != "type"} if radar_voxel_layer else None,
                                     _cfg(radar_voxel_encoder, "PillarFeatureNet", "radar_voxel_encoder") if radar_voxel_encoder else None,
                                     _cfg(radar_middle_encoder, "PointPillarsScatter", "radar_middle_encoder") if radar_middle_encoder else None,
                                     embed_dims=self.pts_bbox_head.embed_dims)
        self.__dict__["radar_encoder"] = enc        # not a registered child: its children carry the detector's names themselves
        self.radar_voxel_layer = enc.radar_voxel_layer
        self.radar_voxel_encoder = enc.radar_voxel_encoder
        self.radar_middle_encoder = enc.radar_middle_encoder
        self.radar_bev_conv = enc.radar_bev_conv

        self._fused_grad = False
        self._weights_touched = False
        self.reset_memory()
        self.eval()

    # ------------------------------------------------------------------------------------------------ the training switch
    @property
    def fused_grad(self):
        """Opt-in to training (module docstring).  Setting it sets ``fused_grad`` on the backbone, both necks and the radar encoder."""
        return self._fused_grad

    @fused_grad.setter
    def fused_grad(self, on):
        self._fused_grad = bool(on)
        for part in (self.img_backbone, self.img_neck, self.img_lss_neck, self.radar_encoder):
            if part is not None and hasattr(part, "fused_grad"):
                part.fused_grad = bool(on)

    # ------------------------------------------------------------------------------------------------ properties of the reference
    @property
    def with_img_neck(self):
        return self.img_neck is not None

    @property
    def with_img_lss_neck(self):
        return self.img_lss_neck is not None

    @property
    def with_pts_bbox(self):
        return self.pts_bbox_head is not None

    def load_state_dict(self, *args, **kwargs):
        self._weights_touched = True
        return super().load_state_dict(*args, **kwargs)

    def train(self, mode=True):
        if mode:
            self._weights_touched = True        # (weights may move from here on: the streaming route re-checks its captured plan)
        super().train(mode)
        self.radar_encoder.training = mode
        return self

    # ------------------------------------------------------------------------------------------------ features
    def _pregrouped_route(self, stage_maps):
        return bool(self.pregrouped) and isinstance(self.img_neck, FPN) and self.img_neck.hip_route(list(stage_maps))

    def extract_img_feat(self, img):
        """img [B*T*N, 3, H, W] -> (pyramid, img_lss_feats [B*T*N, C, h, w]), :107-126 outside training.  The pyramid is the tuple of
        [B*T*N, C, H_i, W_i] of the reference or, on the pregrouped route, the list of [B*T*G, N, H_i, W_i, 64]."""
        BNT = img.shape[0]
        img_feats = self.img_backbone(img)
        if isinstance(img_feats, dict):
            img_feats = list(img_feats.values())
        if self._pregrouped_route(img_feats):
            img_feats_fpn = self.img_neck.forward_pregrouped(list(img_feats))
        else:
            img_feats_fpn = self.img_neck(img_feats)
        img_lss_feats = None
        if self.with_img_lss_neck:
            img_lss_feats = self.img_lss_neck(img_feats[-self.num_lss_fpn:])
            if type(img_lss_feats) in [list, tuple]:
                img_lss_feats = img_lss_feats[0]
            _, output_dim, output_H, output_W = img_lss_feats.shape
            img_lss_feats = img_lss_feats.view(BNT, output_dim, output_H, output_W)
        return img_feats_fpn, img_lss_feats

    def extract_pts_feat(self, radar_points=None):
        """list over B of [n, 7] -> [B, 256, Y, X] (:130-148; the callers' clouds are not modified)."""
        if not self.with_pts_bbox:
            return None
        return self.radar_encoder.extract_pts_feat(radar_points)

    @torch.no_grad()
    def radar_voxelize(self, points):
        """:153-177 -> (voxels, num_points, coors [M, 4])"""
        return self.radar_encoder.radar_voxelize(points)

    def point_maps(self, img, radar_points, img_metas):
        """The radar maps the reference's loader would hand over (RadarPointToMultiViewDepth, downsample 1): radar_points, a list
        over T of lists over B of [n, >= 4] clouds, and ``img_metas[b]['lidar2img']`` -> (radar_depth, radar_rcs) [B, T*N, H, W] on the
        images' device, map t*N + view from frame t's cloud (``point_maps.radar_maps``: HIP on the device, the restatement on CPU)."""
        first = img[0] if isinstance(img, list) else img
        H, W = first.shape[-2:]
        B, T, N = len(img_metas), len(radar_points), self.num_cams
        clouds = [radar_points[t][b].detach().to(first.device, torch.float32) for b in range(B) for t in range(T)]
        points, offsets = pack_clouds(clouds)
        mats = meta_view_table(img_metas, N, frames=T, device=first.device)
        depth, rcs = radar_maps(points, offsets, mats, (H, W), self.img_lss_view_transformer.grid_config)
        return depth.view(B, T * N, H, W), rcs.view(B, T * N, H, W)

    def prepare_raw(self, raw, img_metas, transform, draws=None):
        """What the reference's loader does to the camera frames before the detector sees them (``RandomTransformImage``,
        loaders/pipelines/transforms.py:219-342): raw uint8 [B, T*N, Hr, Wr, 3] (the loader's channel order) and the metas of the raw
        frames -> (img float32 [B, T*N, 3, fH, fW] with values 0..255, img_metas), ready for ``forward_train``, ``simple_test_offline``
        and ``simple_test_online``.  ``transform``: an ``image_geom.RandomTransformImage``; ``draws``: one ``IdaDraw`` per sample, by
        default drawn here in the order of the samples, as the pipeline runs once per sample.  All images go through one launch
        (``image_geom.transform_images``; the numpy route on CPU tensors).  The returned metas are copies whose ``lidar2img`` are
        ``ida_mat @ lidar2img`` (float32 @ the meta's matrix) and whose ``ori_shape`` / ``img_shape`` / ``pad_shape`` are the new
        shape; the caller's metas stay as they are."""
        if raw.dim() != 5 or raw.shape[-1] != 3 or raw.dtype != torch.uint8:
            raise ValueError(f"RaCFormer.prepare_raw: uint8 [B, T*N, H, W, 3] frames expected, got {raw.dtype} {tuple(raw.shape)}")
        B, TN = raw.shape[:2]
        if len(img_metas) != B:
            raise ValueError(f"RaCFormer.prepare_raw: {len(img_metas)} metas for {B} samples")
        draws = [transform.draw() for _ in range(B)] if draws is None else list(draws)
        if len(draws) != B:
            raise ValueError(f"RaCFormer.prepare_raw: {len(draws)} draws for {B} samples")
        img = transform_images(raw.reshape(B * TN, *raw.shape[2:]).contiguous(), draws, out="f32_chw")
        metas = []
        for meta, draw in zip(img_metas, draws):
            mat = ida_mat(draw)
            shape = [tuple(img.shape[-2:]) + (3,)] * TN
            metas.append(dict(meta, lidar2img=[mat @ m for m in meta['lidar2img']], ori_shape=shape, img_shape=list(shape),
                              pad_shape=list(shape)))
        return img.view(B, TN, *img.shape[1:]), metas

    def prepare_bev_aug(self, img_metas, radar_points, points=None, gt_bboxes_3d=None, transform=None, draws=None):
        """The loader's stage between ``prepare_raw`` and the point maps (``RaCGlobalRotScaleTransImage``,
        loaders/pipelines/transforms.py:398-464): one rotation about z and one scaling of the whole scene per sample.  ``radar_points``:
        a list over T of lists over B of [n, 7]; ``points``: a list over B of lidar clouds; ``gt_bboxes_3d``: a list over B of [n, 9]
        (or [n, 7]) boxes, tensors or objects with ``.tensor`` -> (img_metas, radar_points, points, gt_bboxes_3d), ready for
        ``forward_train(radar_depth=None, radar_rcs=None, gt_depth=None, points=...)``.  ``transform``: a
        ``bev_aug.RaCGlobalRotScaleTransImage`` (by default the recipe's); ``draws``: one ``BevDraw`` per sample, by default drawn here
        in the order of the samples.  All clouds and boxes go through one launch (``bev_aug.transform_batch``; the torch route on CPU
        tensors) and come back as views into packed tensors, the clouds in the nesting they came in, the boxes as plain tensors.  The
        returned metas are copies whose ``lidar2img`` are ``bev_aug.view_mats``'; the caller's metas, clouds and boxes stay as they are."""
        B = len(img_metas)
        transform = RaCGlobalRotScaleTransImage() if transform is None else transform
        draws = [transform.draw() for _ in range(B)] if draws is None else list(draws)
        if len(draws) != B:
            raise ValueError(f"RaCFormer.prepare_bev_aug: {len(draws)} draws for {B} samples")
        boxes = None if gt_bboxes_3d is None else [b if isinstance(b, torch.Tensor) else b.tensor for b in gt_bboxes_3d]
        radar, points, boxes = transform_batch(radar_points, points, boxes, draws)
        metas = [dict(meta, lidar2img=view_mats(meta['lidar2img'], draw)) for meta, draw in zip(img_metas, draws)]
        return metas, radar, points, boxes

    def _maps_or_built(self, img, radar_points, radar_depth, radar_rcs, img_metas):
        if (radar_depth is None) != (radar_rcs is None):
            raise ValueError("RaCFormer: radar_depth and radar_rcs go together: pass both, or neither to have them made from radar_points")
        if radar_depth is None:
            return self.point_maps(img, radar_points, img_metas)
        return radar_depth, radar_rcs

    def extract_feat(self, img, radar_points, radar_depth=None, radar_rcs=None, img_metas=None):
        """The eval branch of :179-348.  img [B, T*N, 3, H, W], radar_points a list over T of lists over B of [n, 7], radar_depth /
        radar_rcs [B, T*N, (1,) H, W] -- or both None: made from radar_points and the metas' lidar2img (``point_maps``) -> (img_feats:
        per level [B, T*N, C, H_i, W_i] -- or [B*T*G, N, H_i, W_i, 64], pregrouped --,
        all_bev_feats [B, T, C, Y, X], radar_bev_feats [B, T, 256, Y, X], depth of frame 0 [B*N, D, h, w])."""
        radar_depth, radar_rcs = self._maps_or_built(img, radar_points, radar_depth, radar_rcs, img_metas)
        if self.training:
            if not self.fused_grad:
                raise NotImplementedError(TRAINING_MESSAGE)
            if self.stop_prev_grad > 0:
                raise NotImplementedError("RaCFormer: stop_prev_grad > 0 in training mode is not implemented (the reference's branch cannot "
                                          "run: it calls the view transformer with three arguments and hands all frames' clouds to "
                                          "extract_pts_feat)")
            return self._extract_feat_train(img, radar_points, radar_depth, radar_rcs, img_metas)
        with torch.no_grad():
            return self._extract_feat(img, radar_points, radar_depth, radar_rcs, img_metas)

    @contextlib.contextmanager
    def _branches_eval(self):
        """The radar branch and the view transformer in eval mode for the block, their modes restored afterwards (frames 1 .. T-1 of a
        training step; nothing else of the detector is touched)."""
        enc = self.radar_encoder
        roots = [self.img_lss_view_transformer, self.radar_voxel_layer, self.radar_voxel_encoder, self.radar_middle_encoder, self.radar_bev_conv]
        was = [(m, m.training) for root in roots if isinstance(root, nn.Module) for m in root.modules()] + [(enc, enc.training)]
        for m, _ in was:
            m.training = False
        try:
            yield
        finally:
            for m, t in was:
                m.training = t

    def _extract_feat_train(self, img, radar_points, radar_depth, radar_rcs, img_metas):
        """The training branch of :179-348 (``stop_prev_grad == 0``; module docstring).  Returns the reference's four results with
        their graph: the pyramid [B, T*N, C, H_i, W_i] per level, all_bev_feats [B, T, C, Y, X], radar_bev_feats, frame 0's depth logits."""
        if isinstance(img, list):
            img = torch.stack(img, dim=0)
        assert img.dim() == 5
        B, NT, C, H, W = img.size()
        N = self.num_cams
        T = NT // N
        img = img.reshape(B * NT, C, H, W).float()
        radar_depth = radar_depth.reshape(B * NT, 1, H, W).float()
        radar_rcs = radar_rcs.reshape(B * NT, 1, H, W)

        # the numpy draws in the reference's order: the colour distortion (:199-200), then GridMask on the padded image (:108-109)
        aug = self.data_aug if self.data_aug is not None else {}
        photo = self.color_aug.draw(B * NT) if aug.get('img_color_aug') else None
        div = None
        if self.data_aug is not None:
            for b in range(B):
                img_shape = (H, W, C)
                img_metas[b]['img_shape'] = [img_shape for _ in range(NT)]
                img_metas[b]['ori_shape'] = [img_shape for _ in range(NT)]
            if 'img_pad_cfg' in self.data_aug:
                div = self.data_aug['img_pad_cfg']['size_divisor']
                radar_depth = pad_multiple(radar_depth, img_metas, size_divisor=div)       # (rewrites img_shape / pad_shape of the metas)
                radar_rcs = pad_multiple(radar_rcs, img_metas, size_divisor=div)
        Hp, Wp = radar_depth.shape[-2:]
        grid = self.grid_mask.draw(Hp) if self.use_grid_mask else None
        keep_norm = self.img_backbone.input_norm
        img = prepare_images(img, photo, keep_norm, div, grid)          # one launch on the device: normalised, padded, masked
        H, W = img.shape[-2:]
        radar_depth = radar_depth.reshape(B, N, T, H, W)
        radar_rcs = radar_rcs.reshape(B, N, T, H, W)
        input_shape = img.shape[-2:]
        for img_meta in img_metas:
            img_meta.update(input_shape=input_shape)

        keep_pre = self.pregrouped
        try:
            self.img_backbone.input_norm, self.pregrouped = None, False
            img_feats, img_lss_feats = self.extract_img_feat(img.contiguous())
        finally:
            self.img_backbone.input_norm, self.pregrouped = keep_norm, keep_pre
        self.pts_bbox_head.transformer.decoder.pregrouped = False
        _, C_lss, h, w = img_lss_feats.shape
        img_lss_feats = img_lss_feats.view(B, NT, C_lss, h, w)
        mlp_input = self.img_lss_view_transformer.get_mlp_input(img_metas)

        def frame(i):
            img_meta_b = [dict(lidar2img=img_metas[b]['lidar2img'][i * N:(i + 1) * N],
                               img_shape=img_metas[b]['img_shape'][i * N:(i + 1) * N]) for b in range(B)]
            pts_feats = self.extract_pts_feat(radar_points=radar_points[i])
            bev_feat, depth = self.img_lss_view_transformer(img_lss_feats[:, i * N:(i + 1) * N], radar_depth[:, :, i], radar_rcs[:, :, i],
                                                            img_meta_b, mlp_input[:, i * N:(i + 1) * N])
            return pts_feats, bev_feat, depth

        radar_bev_feats, all_bev_feats, all_depths = [], [], []
        for i in range(T):
            if i == 0:
                with library_deterministic(self.deterministic_forward):     # (DepthNet's torch route: a seeded forward repeats)
                    pts_feats, bev_feat, depth = frame(i)
            else:
                with torch.no_grad(), self._branches_eval():
                    pts_feats, bev_feat, depth = frame(i)
            all_bev_feats.append(bev_feat)
            all_depths.append(depth)
            radar_bev_feats.append(pts_feats)
        all_bev_feats = torch.stack(all_bev_feats, dim=1)
        radar_bev_feats = torch.stack(radar_bev_feats, dim=1)
        img_feats_reshaped = []
        for img_feat in img_feats:
            BN, C, H, W = img_feat.size()
            img_feats_reshaped.append(img_feat.view(B, int(BN / B), C, H, W))
        return img_feats_reshaped, all_bev_feats, radar_bev_feats, all_depths[0]

    def _extract_feat(self, img, radar_points, radar_depth, radar_rcs, img_metas):
        if isinstance(img, list):
            img = torch.stack(img, dim=0)
        assert img.dim() == 5
        B, NT, C, H, W = img.size()
        N = self.num_cams
        T = NT // N
        img = img.reshape(B * NT, C, H, W).float()
        radar_depth = radar_depth.reshape(B * NT, 1, H, W).float()
        radar_rcs = radar_rcs.reshape(B * NT, 1, H, W)

        normalised = False
        if self.data_aug is not None:
            for b in range(B):
                img_shape = (img.shape[2], img.shape[3], img.shape[1])
                img_metas[b]['img_shape'] = [img_shape for _ in range(NT)]
                img_metas[b]['ori_shape'] = [img_shape for _ in range(NT)]
            if 'img_pad_cfg' in self.data_aug:
                div = self.data_aug['img_pad_cfg']['size_divisor']
                if (H % div or W % div) and self.img_backbone.input_norm is not None:
                    # the reference pads the NORMALISED image with zeros: normalise here, and the stem takes the image as it is
                    img, normalised = apply_input_norm(img, self.img_backbone.input_norm), True
                img = pad_multiple(img, img_metas, size_divisor=div)
                radar_depth = pad_multiple(radar_depth, img_metas, size_divisor=div)
                radar_rcs = pad_multiple(radar_rcs, img_metas, size_divisor=div)
        H, W = img.shape[-2:]
        radar_depth = radar_depth.reshape(B, N, T, H, W)        # (the reference's view, :226-227: camera-major)
        radar_rcs = radar_rcs.reshape(B, N, T, H, W)
        input_shape = img.shape[-2:]
        for img_meta in img_metas:
            img_meta.update(input_shape=input_shape)

        keep_norm = self.img_backbone.input_norm
        try:
            if normalised:
                self.img_backbone.input_norm = None
            img_feats, img_lss_feats = self.extract_img_feat(img.contiguous())
        finally:
            self.img_backbone.input_norm = keep_norm
        pregrouped = isinstance(img_feats, list)
        self.pts_bbox_head.transformer.decoder.pregrouped = pregrouped
        _, C_lss, h, w = img_lss_feats.shape
        img_lss_feats = img_lss_feats.view(B, NT, C_lss, h, w)
        mlp_input = self.img_lss_view_transformer.get_mlp_input(img_metas)

        radar_bev_feats, all_bev_feats, all_depths = [], [], []
        for i in range(T):
            img_meta_b = []
            for b in range(B):
                img_meta_b.append(dict(lidar2img=img_metas[b]['lidar2img'][i * N:(i + 1) * N],
                                       img_shape=img_metas[b]['img_shape'][i * N:(i + 1) * N]))
            pts_feats = self.extract_pts_feat(radar_points=radar_points[i])
            bev_feat, depth = self.img_lss_view_transformer(img_lss_feats[:, i * N:(i + 1) * N], radar_depth[:, :, i], radar_rcs[:, :, i],
                                                            img_meta_b, mlp_input[:, i * N:(i + 1) * N])
            all_bev_feats.append(bev_feat)
            all_depths.append(depth)
            radar_bev_feats.append(pts_feats)
        all_bev_feats = torch.stack(all_bev_feats, dim=1)
        radar_bev_feats = torch.stack(radar_bev_feats, dim=1)
        if pregrouped:
            return list(img_feats), all_bev_feats, radar_bev_feats, all_depths[0]
        img_feats_reshaped = []
        for img_feat in img_feats:
            BN, C, H, W = img_feat.size()
            img_feats_reshaped.append(img_feat.view(B, int(BN / B), C, H, W))
        return img_feats_reshaped, all_bev_feats, radar_bev_feats, all_depths[0]

    # ------------------------------------------------------------------------------------------------ entry points
    def forward(self, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(**kwargs)
        return self.forward_test(**kwargs)

    def forward_pts_train(self, pts_feats, bev_feats, radar_bev_feats, depth, gt_bboxes_3d, gt_labels_3d, gt_depth, img_metas,
                          gt_bboxes_ignore=None):
        """:351-382 -> ``loss_depth`` and the head's losses"""
        vt = self.img_lss_view_transformer
        ds = vt.downsample
        if gt_depth.dim() != 4 or gt_depth.shape[0] * gt_depth.shape[1] != depth.shape[0] or gt_depth.shape[2] % ds or gt_depth.shape[3] % ds \
                or (gt_depth.shape[2] // ds, gt_depth.shape[3] // ds) != tuple(depth.shape[2:]):
            raise ValueError(f"RaCFormer.forward_train: gt_depth {tuple(gt_depth.shape)} pooled by {ds} does not give the depth logits' "
                             f"shape {tuple(depth.shape)} (the radar maps are padded inside extract_feat, gt_depth is not: hand it "
                             "over at the padded size)")
        outs = self.pts_bbox_head(pts_feats, bev_feats, radar_bev_feats, img_metas)
        loss_depth = vt.get_depth_loss(gt_depth, depth)
        losses = dict(loss_depth=loss_depth)
        losses.update(self.pts_bbox_head.loss(gt_bboxes_3d, gt_labels_3d, outs))
        return losses

    def lidar_gt_depth(self, points, img, img_metas, pad_hw=None):
        """``gt_depth`` as the reference's loader makes it (PointToMultiViewDepth, downsample 1): points, a list over B of [n, >= 3]
        lidar clouds, and frame 0's views -> [B, N, Hp, Wp] on the images' device (``point_maps.lidar_depth_map``)."""
        first = img[0] if isinstance(img, list) else img
        H, W = first.shape[-2:]
        B, N = len(img_metas), self.num_cams
        pts, offsets = pack_clouds([p.detach().to(first.device, torch.float32) for p in points])
        mats = meta_view_table(img_metas, N, frames=1, device=first.device)
        out = lidar_depth_map(pts, offsets, mats, (H, W), self.img_lss_view_transformer.grid_config, pad_hw=pad_hw)
        return out.view(B, N, *out.shape[-2:])

    def forward_train(self, img_metas=None, gt_bboxes_3d=None, gt_labels_3d=None, gt_depth=None, img=None, radar_points=None,
                      radar_depth=None, radar_rcs=None, gt_bboxes_ignore=None, points=None):
        """:400-441: one training forward -> the dict of losses (``loss_depth``, ``loss_cls``, ``loss_bbox``, ``d{i}.*`` and, with
        denoising queries, the ``*_dn`` keys), each a 0-dim tensor with its graph.  Needs ``fused_grad`` and ``train()``.
        ``radar_depth`` / ``radar_rcs`` None: made from ``radar_points``; ``gt_depth`` None: made from ``points``, a list over B of
        lidar clouds, at the padded size the depth logits stand for."""
        if not self.fused_grad:
            raise NotImplementedError(TRAINING_MESSAGE)
        if not self.training:
            raise RuntimeError("RaCFormer.forward_train: the detector is in eval mode; call train() first")
        self.reset_memory()         # (frames held by the streaming memory, and a captured plan, belong to the weights before this step)
        if gt_depth is None and points is None:
            raise ValueError("RaCFormer.forward_train: gt_depth, or the lidar clouds `points` to make it from, is needed")
        img_feats, bev_feats, radar_bev_feats, depth = self.extract_feat(img, radar_points, radar_depth, radar_rcs, img_metas)
        if gt_depth is None:
            ds = self.img_lss_view_transformer.downsample
            gt_depth = self.lidar_gt_depth(points, img, img_metas, pad_hw=(depth.shape[2] * ds, depth.shape[3] * ds))
        for i in range(len(img_metas)):
            img_metas[i]['gt_bboxes_3d'] = gt_bboxes_3d[i]
            img_metas[i]['gt_labels_3d'] = gt_labels_3d[i]
        return self.forward_pts_train(img_feats, bev_feats, radar_bev_feats, depth, gt_bboxes_3d, gt_labels_3d, gt_depth, img_metas,
                                      gt_bboxes_ignore)

    def forward_test(self, img_metas, img=None, **kwargs):
        for var, name in [(img_metas, 'img_metas')]:
            if not isinstance(var, list):
                raise TypeError('{} must be a list, but got {}'.format(name, type(var)))
        img = [img] if img is None else img
        return self.simple_test(img_metas[0], img[0], **kwargs)

    def simple_test_pts(self, x, bev_feats, radar_bev_feats, img_metas, rescale=False):
        with torch.no_grad():
            outs = self.pts_bbox_head(x, bev_feats, radar_bev_feats, img_metas)
            bbox_list = self.pts_bbox_head.get_bboxes(outs, img_metas[0], rescale=rescale)
        return [bbox3d2result(bboxes, scores, labels) for bboxes, scores, labels in bbox_list]

    def simple_test(self, img_metas, img=None, rescale=False, radar_points=None, radar_depth=None, radar_rcs=None, **kwargs):
        if (radar_depth is None) != (radar_rcs is None):
            raise ValueError("RaCFormer: radar_depth and radar_rcs go together: pass both, or neither to have them made from radar_points")
        return self.simple_test_offline(img_metas, img, rescale, radar_points[0], None if radar_depth is None else radar_depth[0],
                                        None if radar_rcs is None else radar_rcs[0])

    def simple_test_offline(self, img_metas, img=None, rescale=False, radar_points=None, radar_depth=None, radar_rcs=None):
        img_feats, bev_feats, radar_bev_feats, _ = self.extract_feat(img=img, radar_points=radar_points, radar_depth=radar_depth,
                                                                     radar_rcs=radar_rcs, img_metas=img_metas)
        bbox_list = [dict() for _ in range(len(img_metas))]
        bbox_pts = self.simple_test_pts(img_feats, bev_feats, radar_bev_feats, img_metas, rescale=rescale)
        for result_dict, pts_bbox in zip(bbox_list, bbox_pts):
            result_dict['pts_bbox'] = pts_bbox
        return bbox_list

    # ------------------------------------------------------------------------------------------------ streaming
    def reset_memory(self):
        """Empties the frame memory and drops the window buffers and the captured step."""
        if getattr(self, "_plan", None) is not None:
            self._plan.close()
        self.memory, self._window, self._plan, self._plan_sig, self._online_calls = None, None, None, None, 0
        self.stats = dict(calls=0, computed=0, served=0, total_computed=0, total_served=0)

    def _head_weights_sig(self):
        return tuple((p.data_ptr(), p._version) for p in self.pts_bbox_head.parameters())

    def memory_keys(self):
        return list(self.memory.slots) if self.memory is not None else []

    @staticmethod
    def _frame_tensors(img_feats, bev, radar):
        """One frame's extract_feat results as the six tensors a slot holds."""
        return [f.contiguous() for f in img_feats] + [bev[0, 0].contiguous(), radar[0, 0].contiguous()]

    def window_inputs(self, slots, like):
        """The decoder's inputs for the frames in ``slots``: per level T frames back to back -- [T*G, N, H, W, 64] pregrouped,
        [1, T*N, C, H, W] otherwise --, and the two stacks [1, T, C, Y, X]."""
        mem, T = self.memory, len(slots)
        levels = len(mem.rings) - 2

        def shape(k):
            fs = tuple(mem.rings[k].shape[1:])
            if k >= levels:
                return (1, T) + fs
            return (T * fs[0],) + fs[1:] if mem.pregrouped else (1, T * fs[1]) + fs[2:]

        if not like.is_cuda:
            idx = torch.tensor(slots, dtype=torch.long)
            outs = [torch.index_select(r, 0, idx).view(shape(k)) for k, r in enumerate(mem.rings)]
        else:
            from .fused import frames_gather
            win = self._window
            if win is None or len(win) != len(mem.rings) or any(tuple(w.shape) != shape(k) or w.device != mem.rings[k].device
                                                                 for k, w in enumerate(win)):
                if self._plan is not None:
                    self._plan.close()
                    self._plan = None
                win = self._window = [r.new_empty(shape(k)) for k, r in enumerate(mem.rings)]
            outs = frames_gather(mem.rings, win, slots)
        return outs[:levels], outs[levels], outs[levels + 1]

    def simple_test_online(self, img_metas, img=None, rescale=False, radar_points=None, radar_depth=None, radar_rcs=None):
        """:476-557 on the frame memory (module docstring).  img [1, T*N, 3, H, W], radar_points a list over T of lists over B = 1 of
        [n, 7] clouds (as offline), ``img_metas[0]['filename']`` the T*N file names."""
        assert len(img_metas) == 1  # batch_size = 1
        if self.training:
            raise NotImplementedError(TRAINING_MESSAGE)
        B, NT, C, H, W = img.shape
        N = self.num_cams
        img = img.reshape(B, NT // N, N, C, H, W)
        if (radar_depth is None) != (radar_rcs is None):
            raise ValueError("RaCFormer: radar_depth and radar_rcs go together: pass both, or neither to have them made from radar_points")
        built = radar_depth is None         # (then a frame's maps are made when the frame is computed, from its cloud and its metas)
        if not built:
            radar_depth = radar_depth.reshape(B, NT // N, N, 1, H, W)
            radar_rcs = radar_rcs.reshape(B, NT // N, N, 1, H, W)
        img_filenames = img_metas[0]['filename']
        num_frames = len(img_filenames) // N
        img_shape = (H, W, C)
        for k in ('img_shape', 'ori_shape', 'pad_shape'):
            img_metas[0][k] = [img_shape for _ in range(len(img_filenames))]

        n_slots = MEMORY_KEYS - 1 + num_frames       # 15 keys at most before a call, num_frames new ones at most inside it
        if self.memory is not None and n_slots > self.memory.n_slots:
            calls = self.stats
            self.reset_memory()                      # (a longer window than the ring was sized for: a new memory)
            self.stats = calls
        slots, metas_large, computed = [], [], 0
        for i in range(num_frames):
            idx = range(i * N, (i + 1) * N)
            metas_curr = [{k: [v[m] for m in idx] for k, v in img_metas[0].items() if isinstance(v, list)}]
            key = img_filenames[i * N]
            if self.memory is None or key not in self.memory.slots:
                feats, bev, radar, _ = self.extract_feat(img[:, i], [radar_points[i]], None if built else radar_depth[:, i],
                                                         None if built else radar_rcs[:, i], metas_curr)
                tensors = self._frame_tensors(feats, bev, radar)
                pregrouped = self.pts_bbox_head.transformer.decoder.pregrouped
                if self.memory is None or not self.memory.fits(tensors, n_slots, pregrouped):
                    if slots:
                        raise RuntimeError("RaCFormer.simple_test_online: the frames of one window differ in shape or device from the memory's")
                    calls = self.stats
                    self.reset_memory()         # (other shapes, another device, a longer window: a new memory)
                    self.stats = calls
                    self.memory = FrameMemory(n_slots, pregrouped)
                    self.memory.allocate(tensors)
                self.memory.put(key, tensors)
                computed += 1
            slots.append(self.memory.slots[key])
            metas_large.append(metas_curr)

        metas = metas_large[0]
        for other in metas_large[1:]:
            for k, v in other[0].items():
                if isinstance(v, list):
                    metas[0][k].extend(v)

        img_feats, lss_bev_feats, radar_bev_feat = self.window_inputs(slots, img)
        self._online_calls += 1
        self.pts_bbox_head.transformer.decoder.pregrouped = self.memory.pregrouped
        if img.is_cuda and self.capture and self._online_calls > 1:
            if self._plan is not None and self._weights_touched and self._plan_sig != self._head_weights_sig():
                self._plan.close()          # (captured on other weights: its weight-derived operands are stale)
                self._plan = None
            self._weights_touched = False
            if self._plan is None:
                from .graph import CapturedStep
                self._plan = CapturedStep(self.pts_bbox_head, img_feats, lss_bev_feats, radar_bev_feat, metas, decode=False)
                self._plan_sig = self._head_weights_sig()
            with torch.no_grad():
                outs, _ = self._plan.replay(img_metas=metas)
                bbox_list = self.pts_bbox_head.get_bboxes(outs, metas[0], rescale=rescale)
            bbox_pts = [bbox3d2result(bboxes, scores, labels) for bboxes, scores, labels in bbox_list]
        else:
            bbox_pts = self.simple_test_pts(list(img_feats), lss_bev_feats, radar_bev_feat, metas, rescale=rescale)
        result = [dict(pts_bbox=bbox_pts[0])]

        self.memory.evict()
        st = self.stats
        st.update(calls=st["calls"] + 1, computed=computed, served=num_frames - computed,
                  total_computed=st["total_computed"] + computed, total_served=st["total_served"] + num_frames - computed)
        return result
