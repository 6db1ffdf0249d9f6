"""ref_loader.py plus what the reference head's ``loss`` needs (build container only; test infrastructure).

Loads three more reference files -- its two assigners and its match costs -- and stubs the mmdet 2.28.2 names they and
``RaCFormer_head.loss`` import, each restated from mmdet's documented behaviour on torch primitives (no code shared with
``racformer_amd/`` or ``oracle/``):

  mmdet.core                      multi_apply, reduce_mean (one process: the identity)
  mmdet.core.bbox.assigners       AssignResult, BaseAssigner
  mmdet.core.bbox.builder         BBOX_ASSIGNERS (next to ref_loader's BBOX_CODERS)
  mmdet.core.bbox.match_costs     build_match_cost, MATCH_COST with FocalLossCost (and a weight-0 IoUCost that is never called)
  PseudoSampler                   every assigned row is a positive
  FocalLoss(use_sigmoid=True), L1Loss with loss_weight / avg_factor (weight_reduce_loss: sum / (avg_factor + float32 eps))
  DETRHead                        ref_loader's plumbing stub extended by what DETRHead.__init__ sets up for training: assigner from
                                  train_cfg, the pseudo sampler, the two losses, bg_cls_weight = 0, cls_out_channels

One deviation, for a sample WITHOUT boxes: mmdet's SamplingResult reshapes the empty box table to [0,4], which the reference's
``bbox_targets[pos_inds] = pos_gt_bboxes`` then rejects (shape mismatch against [0,9]); the stub keeps the table's own width, so an
empty sample is all background instead of an exception.
"""
import importlib.util
import os
import sys
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

import ref_loader
from ref_loader import REF_ROOT, _Registry, _mod

_BBOX_ASSIGNERS, _MATCH_COST, _LOSSES = _Registry(), _Registry(), _Registry()


def _multi_apply(func, *args, **kwargs):
    from functools import partial
    pfunc = partial(func, **kwargs) if kwargs else func
    return tuple(map(list, zip(*map(pfunc, *args))))


def _reduce_mean(tensor):
    return tensor


class _AssignResult:
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


class _BaseAssigner:
    pass


class _SamplingResult:
    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.pos_bboxes, self.neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]
        self.num_gts = gt_bboxes.shape[0]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        # (mmdet views an empty table as [0,4]; see the module docstring)
        self.pos_gt_bboxes = gt_bboxes[self.pos_assigned_gt_inds.long(), :]
        self.pos_gt_labels = assign_result.labels[pos_inds] if assign_result.labels is not None else None


class _PseudoSampler:
    def sample(self, assign_result, bboxes, gt_bboxes, *args, **kwargs):
        pos_inds = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        return _SamplingResult(pos_inds, neg_inds, bboxes, gt_bboxes, assign_result)


@_MATCH_COST.register_module()
class FocalLossCost:
    def __init__(self, weight=1.0, alpha=0.25, gamma=2, eps=1e-12, binary_input=False):
        assert not binary_input
        self.weight, self.alpha, self.gamma, self.eps = weight, alpha, gamma, eps

    def __call__(self, cls_pred, gt_labels):
        cls_pred = cls_pred.sigmoid()
        neg_cost = -(1 - cls_pred + self.eps).log() * (1 - self.alpha) * cls_pred.pow(self.gamma)
        pos_cost = -(cls_pred + self.eps).log() * self.alpha * (1 - cls_pred).pow(self.gamma)
        cls_cost = pos_cost[:, gt_labels] - neg_cost[:, gt_labels]
        return cls_cost * self.weight


@_MATCH_COST.register_module()
class IoUCost:
    def __init__(self, iou_mode="giou", weight=1.0):
        assert weight == 0.0, "only the config's weight-0 IoU cost is stubbed (the assigners never call it)"
        self.weight = weight


def _weight_reduce_loss(loss, weight=None, reduction="mean", avg_factor=None):
    if weight is not None:
        loss = loss * weight
    assert reduction == "mean"
    if avg_factor is None:
        return loss.mean()
    eps = torch.finfo(torch.float32).eps
    return loss.sum() / (avg_factor + eps)


@_LOSSES.register_module()
class FocalLoss(nn.Module):
    """mmdet FocalLoss on its pure-torch branch (py_sigmoid_focal_loss: what runs for CPU tensors)"""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0, activated=False):
        super().__init__()
        assert use_sigmoid and reduction == "mean" and not activated
        self.use_sigmoid, self.gamma, self.alpha, self.reduction, self.loss_weight = use_sigmoid, gamma, alpha, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        num_classes = pred.size(1)
        target = F.one_hot(target, num_classes=num_classes + 1)[:, :num_classes]
        pred_sigmoid = pred.sigmoid()
        target = target.type_as(pred)
        pt = (1 - pred_sigmoid) * target + pred_sigmoid * (1 - target)
        focal_weight = (self.alpha * target + (1 - self.alpha) * (1 - target)) * pt.pow(self.gamma)
        loss = F.binary_cross_entropy_with_logits(pred, target, reduction="none") * focal_weight
        if weight is not None:
            weight = weight.view(-1, 1)
        return self.loss_weight * _weight_reduce_loss(loss, weight, self.reduction, avg_factor)


@_LOSSES.register_module()
class L1Loss(nn.Module):
    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        assert reduction == "mean"
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        loss = pred.sum() * 0 if target.numel() == 0 else torch.abs(pred - target)
        return self.loss_weight * _weight_reduce_loss(loss, weight, self.reduction, avg_factor)


class _DETRHeadWithLosses(ref_loader._DETRHead):
    """ref_loader._DETRHead plus the training plumbing of mmdet 2.28.2 DETRHead.__init__"""

    def __init__(self, num_classes, in_channels, sync_cls_avg_factor=False, loss_cls=None, loss_bbox=None, loss_iou=None, train_cfg=None,
                 **kwargs):
        super().__init__(num_classes, in_channels, train_cfg=train_cfg, **kwargs)
        self.bg_cls_weight = 0
        self.sync_cls_avg_factor = sync_cls_avg_factor
        if loss_cls is None:
            return
        assert loss_cls.get("class_weight") is None
        if train_cfg:
            assigner = train_cfg["assigner"]
            assert loss_cls["loss_weight"] == assigner["cls_cost"]["weight"] and loss_bbox["loss_weight"] == assigner["reg_cost"]["weight"]
            assert loss_iou is None or loss_iou["loss_weight"] == assigner["iou_cost"]["weight"] == 0.0
            self.assigner = _BBOX_ASSIGNERS.build(assigner)
            self.sampler = _PseudoSampler()
        self.loss_cls, self.loss_bbox = _LOSSES.build(loss_cls), _LOSSES.build(loss_bbox)
        self.cls_out_channels = num_classes if self.loss_cls.use_sigmoid else num_classes + 1


_FILES = [
    ("models.bbox.match_costs.match_cost", "models/bbox/match_costs/match_cost.py"),
    ("models.bbox.assigners.hungarian_assigner_3d", "models/bbox/assigners/hungarian_assigner_3d.py"),
    ("models.bbox.assigners.polar_hungarian_assigner_3d", "models/bbox/assigners/polar_hungarian_assigner_3d.py"),
]


def load_reference():
    """ref_loader.load_reference() with the head able to run ``loss``; call it before anything else loads the reference."""
    assert "models.racformer_head" not in sys.modules, "load the loss-capable reference first: the head binds its imports when loaded"
    ref_loader._install_stubs()
    core = sys.modules["mmdet.core"]
    core.multi_apply, core.reduce_mean = _multi_apply, _reduce_mean
    sys.modules["mmdet.core.bbox.builder"].BBOX_ASSIGNERS = _BBOX_ASSIGNERS
    _mod("mmdet.core.bbox.assigners", AssignResult=_AssignResult, BaseAssigner=_BaseAssigner)
    _mod("mmdet.core.bbox.match_costs", build_match_cost=_MATCH_COST.build)
    _mod("mmdet.core.bbox.match_costs.builder", MATCH_COST=_MATCH_COST)
    sys.modules["mmdet.models.dense_heads"].DETRHead = _DETRHeadWithLosses
    ref = ref_loader.load_reference()
    for pkg, sub in (("models.bbox.match_costs", "models/bbox/match_costs"), ("models.bbox.assigners", "models/bbox/assigners")):
        if pkg not in sys.modules:
            m = types.ModuleType(pkg)
            m.__path__ = [os.path.join(REF_ROOT, sub)]
            sys.modules[pkg] = m
    for name, rel in _FILES:
        if name not in sys.modules:
            spec = importlib.util.spec_from_file_location(name, os.path.join(REF_ROOT, rel))
            mod = importlib.util.module_from_spec(spec)
            sys.modules[name] = mod
            spec.loader.exec_module(mod)
        setattr(ref, name.split(".")[-1], sys.modules[name])
    return ref
