"""Match costs, Hungarian assigners and losses of ``RaCFormer_head.loss``.

Counterparts of the reference's ``models/bbox/match_costs/match_cost.py`` (BBox3DL1Cost, ThetaL1Cost),
``models/bbox/assigners/{hungarian,polar_hungarian}_assigner_3d.py`` and of the mmdet 2.28.2 pieces its config names
(FocalLossCost, FocalLoss, L1Loss, restated from their documented behaviour): same names, constructor arguments and results.
The classes here are the plain-torch route (any device; the assignment is solved on the host by rac_lsap_host, no scipy);
``head_loss_sums`` is what the head's fused route differentiates through: rac_det_loss_fwd under a torch.autograd.Function."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .bbox_utils import normalize_bbox, xy2theta_d_coods

_EPS32 = float(torch.finfo(torch.float32).eps)


# ------------------------------------------------------------------------------------------------ match costs
class FocalLossCost:
    """mmdet FocalLossCost: (pos - neg)[:, gt_labels] * weight on sigmoid(cls_pred) [Q,C] -> [Q,G]"""

    def __init__(self, weight=1.0, alpha=0.25, gamma=2, eps=1e-12):
        self.weight, self.alpha, self.gamma, self.eps = weight, alpha, gamma, eps

    def __call__(self, cls_pred, gt_labels):
        p = cls_pred.sigmoid()
        neg = -(1 - p + self.eps).log() * (1 - self.alpha) * p.pow(self.gamma)
        pos = -(p + self.eps).log() * self.alpha * (1 - p).pow(self.gamma)
        return (pos[:, gt_labels] - neg[:, gt_labels]) * self.weight


class BBox3DL1Cost:
    """match_cost.py:6-27"""

    def __init__(self, weight=1.0):
        self.weight = weight

    def __call__(self, bbox_pred, gt_bboxes):
        return torch.cdist(bbox_pred, gt_bboxes, p=1) * self.weight


class ThetaL1Cost:
    """match_cost.py:30-64: L1 between the polar angles (turns) of the centres, wrapped to [0, 0.5].  The centres are normalised
    with the class's own pc_range, whatever the model's is.  (The reference writes the normalised centres back into its
    arguments, which are temporaries of the assigner; here the arguments are left alone.)"""
    pc_range = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]

    def __init__(self, weight=1.0):
        self.weight = weight

    def theta(self, boxes):
        pc = self.pc_range
        xy = torch.stack([(boxes[..., 0] - pc[0]) / (pc[3] - pc[0]), (boxes[..., 1] - pc[1]) / (pc[4] - pc[1])], dim=-1)
        return xy2theta_d_coods(xy)[..., 0:1]

    def __call__(self, bbox_pred, gt_bboxes):
        theta_cost = torch.cdist(self.theta(bbox_pred), self.theta(gt_bboxes), p=1)
        return torch.abs(torch.remainder(theta_cost + 0.5, 1) - 0.5) * self.weight


class _ZeroIoUCost:
    def __init__(self, weight=0.0):
        if weight:
            raise NotImplementedError("racformer_amd: IoU match costs are not built (the reference's configs weigh them 0)")
        self.weight = weight


MATCH_COSTS = {"FocalLossCost": FocalLossCost, "BBox3DL1Cost": BBox3DL1Cost, "ThetaL1Cost": ThetaL1Cost, "IoUCost": _ZeroIoUCost,
               "IoU3DCost": _ZeroIoUCost}


def build_match_cost(cfg):
    if not isinstance(cfg, dict):
        return cfg
    cfg = dict(cfg)
    kind = cfg.pop("type")
    if kind not in MATCH_COSTS:
        raise NotImplementedError(f"racformer_amd: match cost {kind!r} is not built")
    return MATCH_COSTS[kind](**cfg)


# ------------------------------------------------------------------------------------------------ assigners
class HungarianAssigner3D:
    """hungarian_assigner_3d.py: cost = cls_cost + reg_cost on the code-weighted normalised boxes, nan_to_num(100, 100, -100), one
    query per ground-truth box at minimum total cost."""
    polar = False

    def __init__(self, cls_cost=dict(type="ClassificationCost", weight=1.0), reg_cost=dict(type="BBoxL1Cost", weight=1.0),
                 iou_cost=dict(type="IoUCost", weight=0.0), pc_range=None):
        self.cls_cost, self.reg_cost, self.iou_cost = build_match_cost(cls_cost), build_match_cost(reg_cost), build_match_cost(iou_cost)
        self.pc_range = pc_range

    def fusable(self):
        """the device route computes FocalLossCost(alpha 0.25, gamma 2, eps 1e-12) + BBox3DL1Cost (+ ThetaL1Cost)"""
        c = self.cls_cost
        return type(c) is FocalLossCost and (c.alpha, c.gamma, c.eps) == (0.25, 2, 1e-12) and type(self.reg_cost) is BBox3DL1Cost \
            and (not self.polar or type(self.theta_cost) is ThetaL1Cost)

    def cost(self, bbox_pred, cls_pred, gt_bboxes, gt_labels, code_weights=None, with_velo=False):
        """the [Q,G] cost matrix the solver sees"""
        cls_cost = self.cls_cost(cls_pred, gt_labels)
        normalized_gt_bboxes = normalize_bbox(gt_bboxes)
        if code_weights is not None:
            bbox_pred = bbox_pred * code_weights
            normalized_gt_bboxes = normalized_gt_bboxes * code_weights
        if with_velo:
            reg_cost = self.reg_cost(bbox_pred, normalized_gt_bboxes)
        else:
            reg_cost = self.reg_cost(bbox_pred[:, :8], normalized_gt_bboxes[:, :8])
        cost = cls_cost + reg_cost
        if self.polar:
            cost = cost + self.theta_cost(bbox_pred, normalized_gt_bboxes)
        return torch.nan_to_num(cost.detach(), nan=100.0, posinf=100.0, neginf=-100.0)

    def assign(self, bbox_pred, cls_pred, gt_bboxes, gt_labels, gt_bboxes_ignore=None, code_weights=None, with_velo=False):
        """-> (assigned_gt_inds [Q] long: 0 background, 1-based index of the matched box; assigned_labels [Q] long: the box's
        label, -1 on background rows) -- the two fields of the reference's AssignResult that its head reads"""
        assert gt_bboxes_ignore is None, "Only case when gt_bboxes_ignore is None is supported."
        num_gts, num_bboxes = gt_bboxes.size(0), bbox_pred.size(0)
        assigned_gt_inds = bbox_pred.new_full((num_bboxes,), -1, dtype=torch.long)
        assigned_labels = bbox_pred.new_full((num_bboxes,), -1, dtype=torch.long)
        if num_gts == 0 or num_bboxes == 0:
            if num_gts == 0:
                assigned_gt_inds[:] = 0
            return assigned_gt_inds, assigned_labels
        from .fused import lsap_host
        cost = self.cost(bbox_pred, cls_pred, gt_bboxes, gt_labels, code_weights, with_velo).float().cpu()
        _, matched_gt, _, _, _ = lsap_host(cost_qg=cost)
        matched_gt = matched_gt.to(bbox_pred.device).long()
        pos = matched_gt >= 0
        assigned_gt_inds = torch.where(pos, matched_gt + 1, torch.zeros_like(matched_gt))
        assigned_labels = torch.where(pos, gt_labels.long()[matched_gt.clamp(min=0)], assigned_labels)
        return assigned_gt_inds, assigned_labels


class PolarHungarianAssigner3D(HungarianAssigner3D):
    """polar_hungarian_assigner_3d.py: the same with ThetaL1Cost added"""
    polar = True

    def __init__(self, cls_cost=dict(type="ClassificationCost", weight=1.0), reg_cost=dict(type="BBoxL1Cost", weight=1.0),
                 theta_cost=dict(type="ThetaL1Cost", weight=1.0), iou_cost=dict(type="IoUCost", weight=0.0), pc_range=None):
        super().__init__(cls_cost, reg_cost, iou_cost, pc_range)
        self.theta_cost = build_match_cost(theta_cost)


ASSIGNERS = {"HungarianAssigner3D": HungarianAssigner3D, "PolarHungarianAssigner3D": PolarHungarianAssigner3D}


def build_assigner(cfg):
    if not isinstance(cfg, dict):
        return cfg
    cfg = dict(cfg)
    kind = cfg.pop("type")
    if kind not in ASSIGNERS:
        raise NotImplementedError(f"racformer_amd: assigner {kind!r} is not built")
    return ASSIGNERS[kind](**cfg)


# ------------------------------------------------------------------------------------------------ losses
def _reduce(loss, avg_factor):
    """mmdet weight_reduce_loss with reduction='mean': the sum over (avg_factor + float32 eps), the plain mean without one"""
    if avg_factor is None:
        return loss.mean()
    return loss.sum() / (avg_factor + _EPS32)


class FocalLoss(nn.Module):
    """mmdet FocalLoss(use_sigmoid=True), reduction 'mean': pred [N,C] logits, target [N] labels with C = background."""

    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction="mean", loss_weight=1.0, activated=False):
        super().__init__()
        if not use_sigmoid or reduction != "mean" or activated:
            raise NotImplementedError("racformer_amd: FocalLoss is built for use_sigmoid=True, reduction='mean', activated=False")
        self.use_sigmoid, self.gamma, self.alpha, self.reduction, self.loss_weight = use_sigmoid, gamma, alpha, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        C = pred.size(1)
        t = F.one_hot(target, num_classes=C + 1)[:, :C].type_as(pred)
        p = pred.sigmoid()
        pt = (1 - p) * t + p * (1 - t)
        focal_weight = (self.alpha * t + (1 - self.alpha) * (1 - t)) * pt.pow(self.gamma)
        loss = F.binary_cross_entropy_with_logits(pred, t, reduction="none") * focal_weight
        if weight is not None:
            loss = loss * weight.view(-1, 1)
        return self.loss_weight * _reduce(loss, avg_factor)


class L1Loss(nn.Module):
    """mmdet L1Loss, reduction 'mean': |pred - target| * weight; pred.sum() * 0 for an empty target."""

    def __init__(self, reduction="mean", loss_weight=1.0):
        super().__init__()
        if reduction != "mean":
            raise NotImplementedError("racformer_amd: L1Loss is built for reduction='mean'")
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None):
        loss = pred.sum() * 0 if target.numel() == 0 else torch.abs(pred - target)
        if weight is not None:
            loss = loss * weight
        return self.loss_weight * _reduce(loss, avg_factor)


LOSSES = {"FocalLoss": FocalLoss, "L1Loss": L1Loss}


def build_loss(cfg):
    if cfg is None or not isinstance(cfg, dict):
        return cfg
    cfg = dict(cfg)
    kind = cfg.pop("type")
    if kind not in LOSSES:
        raise NotImplementedError(f"racformer_amd: loss {kind!r} is not built")
    return LOSSES[kind](**cfg)


# ------------------------------------------------------------------------------------------------ the fused sums
class _DetLossSums(torch.autograd.Function):
    """rac_det_loss_fwd: the raw per-layer sums [L,2] (focal, L1); the kernel's unit gradients are kept and scaled by
    grad_output[l, k] in backward -- averaging, loss weights and nan_to_num stay torch operations on the [L] vectors."""

    @staticmethod
    def forward(ctx, logits, boxes, target, gt_boxes, gt_labels, code_weights, alpha, gamma):
        from .fused import det_loss_fused
        sums, g_logits, g_boxes = det_loss_fused(logits, boxes, target, gt_boxes, gt_labels, code_weights, alpha, gamma)
        ctx.save_for_backward(g_logits, g_boxes)
        return sums

    @staticmethod
    def backward(ctx, grad_sums):
        g_logits, g_boxes = ctx.saved_tensors
        return (g_logits * grad_sums[:, 0].reshape(-1, 1, 1) if ctx.needs_input_grad[0] else None,
                g_boxes * grad_sums[:, 1].reshape(-1, 1, 1) if ctx.needs_input_grad[1] else None, None, None, None, None, None, None)


def head_loss_sums(logits, boxes, target, gt_boxes, gt_labels, code_weights, alpha=0.25, gamma=2.0):
    """logits [L,R,C], boxes [L,R,10] (CUDA float32, may require grad); target [L,R] int32 or None; -> sums [L,2]"""
    return _DetLossSums.apply(logits.contiguous(), boxes.contiguous(), target, gt_boxes, gt_labels, code_weights, alpha, gamma)
