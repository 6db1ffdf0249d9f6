"""Counterparts of ``RaCFormer_head`` (models/racformer_head.py:13-262, 488-507)
and ``NMSFreeCoder`` (models/bbox/coders/nms_free_coder.py:8-110): same names, constructor
arguments, ``forward`` / ``get_bboxes`` / ``decode`` behaviour and ``state_dict`` keys
(``init_query_bbox.weight``, ``label_enc.weight``, ``code_weights``, ``transformer.*``).
Training mode builds the query-denoising inputs (``prepare_for_dn_input``), runs the decoder under their attention mask and
returns the reference's dict with ``dn_mask_dict``.  ``loss`` (racformer_head.py:264-485) is built when the constructor gets
``loss_cls``, ``loss_bbox`` and ``train_cfg['assigner']``: on CUDA float32 outputs as three HIP launches for all layers and
samples (match costs, assignment, focal + L1) plus one for the denoising rows, without a host read-back; ``loss_unfused`` is the
reference's per-layer, per-sample route.  A head built without them raises from ``loss``."""
import math

import torch
import torch.nn as nn

from .bbox_utils import const_tensor, denormalize_bbox, encode_bbox, normalize_bbox, xy2theta_d_coods
from .losses import FocalLoss, L1Loss, build_assigner, build_loss, head_loss_sums
from .transformer import RaCFormerTransformer

_EPS32 = float(torch.finfo(torch.float32).eps)


def multi_apply(func, *args):
    """mmdet.core.multi_apply: map, then transpose the results"""
    return tuple(map(list, zip(*map(func, *args))))


def reduce_mean(tensor):
    """mmdet.core.reduce_mean: the mean over the ranks (the tensor itself outside torch.distributed)"""
    if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
        return tensor
    tensor = tensor.clone()
    torch.distributed.all_reduce(tensor.div_(torch.distributed.get_world_size()), op=torch.distributed.ReduceOp.SUM)
    return tensor


def plain_gt_boxes(gt, device):
    """[n,9] (gravity centre, w, l, h, yaw, vx, vy) from mmdet3d-style boxes (``.gravity_center``, ``.tensor``) or a plain tensor"""
    if not isinstance(gt, torch.Tensor):
        gt = torch.cat((gt.gravity_center, gt.tensor[:, 3:]), dim=1)
    return gt.to(device)


class NMSFreeCoder:
    """nms_free_coder.py:8-110"""

    def __init__(self, pc_range, voxel_size=None, post_center_range=None, max_num=100, score_threshold=None,
                 num_classes=10):
        self.pc_range, self.voxel_size, self.post_center_range = pc_range, voxel_size, post_center_range
        self.max_num, self.score_threshold, self.num_classes = max_num, score_threshold, num_classes

    def topk_fixed(self, cls_scores, bbox_preds):
        """The shape-static half of decode_single (:48-57 + masks :61-69): no boolean indexing,
        so nothing synchronises with the host.  -> boxes [K,9], scores [K], labels [K], keep [K]."""
        scores, indexs = cls_scores.sigmoid().view(-1).topk(self.max_num)
        labels = indexs % self.num_classes
        bbox_index = torch.div(indexs, self.num_classes, rounding_mode="trunc")
        boxes = denormalize_bbox(bbox_preds[bbox_index])
        if self.post_center_range is None:
            raise NotImplementedError("Need to reorganize output as a batch, only support "
                                      "post_center_range is not None for now!")
        limit = const_tensor(boxes, self.post_center_range)
        keep = (boxes[..., :3] >= limit[:3]).all(1) & (boxes[..., :3] <= limit[3:]).all(1)
        if self.score_threshold:
            keep &= scores > self.score_threshold
        return boxes, scores, labels, keep

    def decode_single(self, cls_scores, bbox_preds):
        boxes, scores, labels, keep = self.topk_fixed(cls_scores, bbox_preds)
        return {"bboxes": boxes[keep], "scores": scores[keep], "labels": labels[keep]}

    def decode(self, preds_dicts):
        all_cls_scores = preds_dicts["all_cls_scores"][-1]
        all_bbox_preds = preds_dicts["all_bbox_preds"][-1]
        return [self.decode_single(all_cls_scores[i], all_bbox_preds[i]) for i in range(all_cls_scores.size(0))]


class RaCFormer_head(nn.Module):
    """models/racformer_head.py.  ``transformer`` is a config dict (``type='RaCFormerTransformer'``, as in
    configs/racformer_r50_nuimg_704x256_f8.py:152-166) or a module; ``bbox_coder`` a config dict (``type='NMSFreeCoder'``) or an
    instance; ``loss_cls`` (FocalLoss, use_sigmoid=True), ``loss_bbox`` (L1Loss) and ``train_cfg['assigner']``
    (PolarHungarianAssigner3D / HungarianAssigner3D) config dicts as in the same file (:180-199) or instances -- without them the
    head is an inference head and ``loss`` raises."""

    def __init__(self, *args, num_classes, in_channels, num_query=900, num_clusters=5, transformer=None,
                 bbox_coder=None, code_size=10, code_weights=[1.0] * 10, query_denoising=True,
                 query_denoising_groups=10, train_cfg=dict(), test_cfg=dict(max_per_img=100), loss_cls=None, loss_bbox=None,
                 loss_iou=None, sync_cls_avg_factor=False, **kwargs):
        super().__init__()
        # mmdet's DETRHead: the background weight of the classification term is 0 with FocalLoss (class_weight is not given)
        self.bg_cls_weight, self.sync_cls_avg_factor, self.cls_out_channels = 0, sync_cls_avg_factor, num_classes
        if isinstance(loss_iou, dict) and loss_iou.get("loss_weight", 1.0) != 0:
            raise NotImplementedError("racformer_amd: an IoU loss is not built (the reference's configs weigh it 0)")
        self.loss_cls, self.loss_bbox = build_loss(loss_cls), build_loss(loss_bbox)
        self.assigner = build_assigner(train_cfg["assigner"]) if train_cfg and "assigner" in train_cfg else None
        self.num_classes, self.in_channels, self.embed_dims = num_classes, in_channels, in_channels
        self.num_query, self.num_clusters, self.code_size = num_query, num_clusters, code_size
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        if isinstance(transformer, dict):
            tcfg = dict(transformer)
            assert tcfg.pop("type", "RaCFormerTransformer") == "RaCFormerTransformer"
            transformer = RaCFormerTransformer(**tcfg)
        self.transformer = transformer
        if isinstance(bbox_coder, dict):
            ccfg = dict(bbox_coder)
            assert ccfg.pop("type", "NMSFreeCoder") == "NMSFreeCoder"
            bbox_coder = NMSFreeCoder(**ccfg)
        self.bbox_coder = bbox_coder
        self.pc_range = self.bbox_coder.pc_range
        self.code_weights = nn.Parameter(torch.tensor(code_weights), requires_grad=False)
        # query denoising (racformer_head.py:45-49)
        self.dn_enabled = query_denoising
        self.dn_group_num = query_denoising_groups
        self.dn_weight = 1.0
        self.dn_bbox_noise_scale = 0.5
        self.dn_label_noise_scale = 0.5
        self._init_layers()

    def _init_layers(self):
        """racformer_head.py:51-63: polar query grid (num_query//num_clusters rays x clusters)."""
        self.init_query_bbox = nn.Embedding(self.num_query, 10)
        self.label_enc = nn.Embedding(self.num_classes + 1, self.embed_dims - 1)
        with torch.no_grad():
            nn.init.constant_(self.init_query_bbox.weight[:, 2:3], 0.5)
            nn.init.zeros_(self.init_query_bbox.weight[:, 8:10])
            nn.init.constant_(self.init_query_bbox.weight[:, 5:6], 0.2)
            self.init_query_bbox.weight[:, :2] = self.generate_points().reshape(-1, 2)

    def init_weights(self):
        self.transformer.init_weights()

    def generate_points(self):
        """Polar query grid of racformer_head.py:69-79: ``num_query // num_clusters`` rays (theta in [0,1), 0
        excluded at the top end) times ``num_clusters`` ranges strictly inside (0,1); row-major (ray, cluster)."""
        rays = self.num_query // self.num_clusters
        theta = torch.linspace(0, 1, rays + 1)[:rays]
        rng = torch.linspace(0, 1, self.num_clusters + 2, dtype=torch.float)[1:self.num_clusters + 1]
        grid = torch.stack(torch.meshgrid(theta, rng, indexing="ij"), dim=-1)       # [rays, clusters, 2]
        return grid.reshape(-1, 2)

    def eval_queries(self, B):
        """The eval branch of prepare_for_dn_input (:142-145, :241-245) -> (query_bbox [B,Q,10], query_feat [B,Q,E], query_key).
        The initial queries depend on the embeddings only: built once per (weights, batch size) in eval, not per forward (four
        small launches per step otherwise); the decoder never writes into its inputs.  ``query_key`` names exactly these cached
        tensors -- the key under which the decoder's layer 0 keeps what it computes from them alone
        (RaCFormerTransformerDecoderLayer.layer0_block); None while autograd is recording (fresh tensors, nothing is cached)."""
        Q = self.num_query
        wq, wl = self.init_query_bbox.weight, self.label_enc.weight
        sig = (wq.data_ptr(), wq._version, wl.data_ptr(), wl._version, str(wq.device), B)
        hit = getattr(self, "_init_queries", None)
        if hit is None or hit[0] != sig or torch.is_grad_enabled():
            query_bbox = wq.view(1, Q, 10).repeat(B, 1, 1)
            feat = wl[self.num_classes].repeat(Q, 1)
            query_feat = torch.cat([feat, feat.new_zeros(Q, 1)], dim=1).repeat(B, 1, 1)
            if not torch.is_grad_enabled():
                self._init_queries = (sig, query_bbox, query_feat)
        else:
            _, query_bbox, query_feat = hit
        return query_bbox, query_feat, (("init_queries",) + sig if not torch.is_grad_enabled() else None)

    def forward(self, mlvl_feats, lss_bev_feats, radar_bev_feats, img_metas):
        """racformer_head.py:82-134.  Eval mode: the eval branch of prepare_for_dn_input (:142-145, :241-245) with cached initial
        queries and the fused output tail.  Training mode: forward_training."""
        if self.training:
            return self.forward_training(mlvl_feats, lss_bev_feats, radar_bev_feats, img_metas)
        query_bbox, query_feat, query_key = self.eval_queries(lss_bev_feats.shape[0])
        pc = self.pc_range
        if lss_bev_feats.is_cuda and self.code_size == 10 and not torch.is_grad_enabled():
            # nan_to_num of both outputs, the centre's scaling to metres and the column reorder: one HIP launch instead of five
            from .fused import head_finish_fused
            cls_scores, bbox_xy = self.transformer(query_bbox, query_feat, mlvl_feats, lss_bev_feats, radar_bev_feats,
                                                   attn_mask=None, img_metas=img_metas, raw=True, query_key=query_key)
            if cls_scores.dtype == torch.float32 and bbox_xy.dtype == torch.float32:
                cls_scores, bbox_preds = head_finish_fused(cls_scores.contiguous(), bbox_xy.contiguous(), pc)
                return {"all_cls_scores": cls_scores, "all_bbox_preds": bbox_preds, "enc_cls_scores": None, "enc_bbox_preds": None}
            cls_scores, bbox_preds = torch.nan_to_num(cls_scores), torch.nan_to_num(bbox_xy)
        else:
            cls_scores, bbox_preds = self.transformer(query_bbox, query_feat, mlvl_feats, lss_bev_feats,
                                                      radar_bev_feats, attn_mask=None, img_metas=img_metas, query_key=query_key)
        lo = const_tensor(bbox_preds, pc[0:3])
        span = const_tensor(bbox_preds, [pc[3] - pc[0], pc[4] - pc[1], pc[5] - pc[2]])
        xyz = bbox_preds[..., 0:3] * span + lo
        bbox_preds = torch.cat([xyz[..., 0:2], bbox_preds[..., 3:5], xyz[..., 2:3], bbox_preds[..., 5:10]], dim=-1)
        return {"all_cls_scores": cls_scores, "all_bbox_preds": bbox_preds, "enc_cls_scores": None,
                "enc_bbox_preds": None}

    def forward_training(self, mlvl_feats, lss_bev_feats, radar_bev_feats, img_metas):
        """racformer_head.py:82-134 in ``training`` mode: the denoising queries in front of the matching queries, the decoder under
        their attention mask (packed once, the fused masked self-attention in all six layers), the outputs split at ``pad_size``
        -> the reference's dict, with ``dn_mask_dict`` when there are denoising queries.  With ``query_denoising=False`` (or no
        ground-truth box in the batch) the decoder runs with ``attn_mask=None``.  Dropout is not applied in training mode either:
        the layers carry none (INTEGRATION.md records this for the attention)."""
        B = lss_bev_feats.shape[0]
        query_bbox = self.init_query_bbox.weight.clone().view(1, self.num_query, 10).repeat(B, 1, 1)
        query_bbox, query_feat, attn_mask, mask_dict = self.prepare_for_dn_input(B, query_bbox, self.label_enc, img_metas)
        cls_scores, bbox_preds = self.transformer(query_bbox, query_feat, mlvl_feats, lss_bev_feats, radar_bev_feats,
                                                  attn_mask=attn_mask, img_metas=img_metas)
        pc = self.pc_range
        lo = const_tensor(bbox_preds, pc[0:3])
        span = const_tensor(bbox_preds, [pc[3] - pc[0], pc[4] - pc[1], pc[5] - pc[2]])
        xyz = bbox_preds[..., 0:3] * span + lo
        bbox_preds = torch.cat([xyz[..., 0:2], bbox_preds[..., 3:5], xyz[..., 2:3], bbox_preds[..., 5:10]], dim=-1)
        outs = {"all_cls_scores": cls_scores, "all_bbox_preds": bbox_preds, "enc_cls_scores": None, "enc_bbox_preds": None}
        if mask_dict is not None and mask_dict["pad_size"] > 0:
            pad = mask_dict["pad_size"]
            mask_dict["output_known_lbs_bboxes"] = (cls_scores[:, :, :pad, :], bbox_preds[:, :, :pad, :])
            outs.update(all_cls_scores=cls_scores[:, :, pad:, :], all_bbox_preds=bbox_preds[:, :, pad:, :], dn_mask_dict=mask_dict)
        return outs

    def prepare_for_dn_input(self, batch_size, init_query_bbox, label_enc, img_metas):
        """racformer_head.py:136-247 (after DN-DETR's dn_components and PETRv2's dn head): ``dn_group_num`` noised copies of
        every ground-truth box as extra queries in front of the matching queries, and the bool [Q,Q] mask (True: blocked) that
        keeps the matching queries from seeing them and the groups from seeing each other.
        -> (input_query_bbox [B, pad+Q, 10], input_query_feat [B, pad+Q, E], attn_mask, mask_dict); in eval mode or with
        denoising off: the plain queries, None, None; if no sample has a box: the plain queries, None and a mask_dict with
        ``pad_size == 0``.  ``img_metas[b]['gt_bboxes_3d']``: an object with ``.gravity_center`` and ``.tensor`` (mmdet3d's
        LiDARInstance3DBoxes), or a plain [n,9] tensor (x, y, z, w, l, h, yaw, vx, vy) whose centre is the gravity centre;
        ``['gt_labels_3d']``: an integer tensor.  The random draws come in the reference's order (box noise, label choice, new
        labels), so a seeded run reproduces it.  The number of re-labelled queries is read back by the host (nonzero)."""
        device = init_query_bbox.device
        Q = self.num_query
        init_query_feat = label_enc.weight[self.num_classes].repeat(Q, 1)
        init_query_feat = torch.cat([init_query_feat, torch.zeros([Q, 1], device=device)], dim=1).repeat(batch_size, 1, 1)
        if not (self.training and self.dn_enabled):
            return init_query_bbox, init_query_feat, None, None

        groups = self.dn_group_num
        boxes, labels_per = [], []
        for m in img_metas:
            if "gt_bboxes_3d" not in m or "gt_labels_3d" not in m:
                # (the reference's train pipeline puts both into img_metas; nothing here builds them)
                raise NotImplementedError("racformer_amd: training mode with query denoising needs gt_bboxes_3d and gt_labels_3d "
                                          "in every img_metas entry (the data pipeline that supplies them is not built)")
            gt = m["gt_bboxes_3d"]
            if not isinstance(gt, torch.Tensor):
                gt = torch.cat([gt.gravity_center, gt.tensor[:, 3:]], dim=1)
            boxes.append(gt.to(device))
            labels_per.append(m["gt_labels_3d"].to(device).long())
        known_num = [int(l.shape[0]) for l in labels_per]          # (host integers: no read-back)
        total = sum(known_num)
        labels = torch.cat(labels_per).clone()
        bboxes = torch.cat(boxes).clone()
        batch_idx = torch.cat([torch.full_like(l, i) for i, l in enumerate(labels_per)])
        known_indice = torch.arange(total, device=device).repeat(groups, 1).view(-1)
        known_labels = labels.repeat(groups, 1).view(-1)
        known_bid = batch_idx.repeat(groups, 1).view(-1)
        known_bboxs = bboxes.repeat(groups, 1)
        if total == 0:
            empty = torch.zeros(0, dtype=torch.long, device=device)
            return init_query_bbox, init_query_feat, None, {
                "known_indice": known_indice, "batch_idx": batch_idx, "map_known_indice": empty,
                "known_lbs_bboxes": (known_labels, known_bboxs), "pad_size": 0}
        known_labels_expand = known_labels.clone()
        wlh = known_bboxs[..., 3:6].clone()
        known_bbox_expand = xy2theta_d_coods(encode_bbox(known_bboxs, self.pc_range))

        if self.dn_bbox_noise_scale > 0:        # noise on the box: along the arc, along the ray, in height
            r = 65.0
            rand_prob = torch.rand_like(known_bbox_expand) * 2 - 1.0
            diag = torch.sqrt(wlh[..., 0:1] ** 2 + wlh[..., 1:2] ** 2)
            arc_len_ratio = diag / (2 * math.pi * known_bbox_expand[..., 1:2] * r)
            theta_delta = torch.mul(rand_prob[..., 0:1], arc_len_ratio / 2) * self.dn_bbox_noise_scale * known_bbox_expand[..., 1:2]
            d_delta = torch.mul(rand_prob[..., 1:2], diag / (r * 2)) * self.dn_bbox_noise_scale
            theta = known_bbox_expand[..., 0:1] + theta_delta
            theta = ((theta + 1) * 2 * math.pi % (2 * math.pi)) / (2 * math.pi)
            dist = known_bbox_expand[..., 1:2] + d_delta
            z = known_bbox_expand[..., 2:3] + torch.mul(rand_prob[..., 2:3], wlh[..., 2:3] / (8 * 2)) * self.dn_bbox_noise_scale
            known_bbox_expand = torch.cat([theta, dist, z, known_bbox_expand[..., 3:]], dim=-1)
        known_bbox_expand = torch.cat([known_bbox_expand[..., 0:3].clamp(min=0.0, max=1.0), known_bbox_expand[..., 3:]], dim=-1)
        if self.dn_label_noise_scale > 0:       # noise on the label: about half of them get a random class
            p = torch.rand_like(known_labels_expand.float())
            chosen_indice = torch.nonzero(p < self.dn_label_noise_scale).view(-1)
            new_label = torch.randint_like(chosen_indice, 0, self.num_classes)
            known_labels_expand.scatter_(0, chosen_indice, new_label)
        known_feat_expand = label_enc(known_labels_expand)
        known_feat_expand = torch.cat([known_feat_expand, torch.ones([known_feat_expand.shape[0], 1], device=device)], dim=1)

        dn_single_pad = max(known_num)
        dn_pad_size = dn_single_pad * groups
        dn_query_bbox = torch.zeros([batch_size, dn_pad_size, init_query_bbox.shape[-1]], device=device)
        dn_query_feat = torch.zeros([batch_size, dn_pad_size, self.embed_dims], device=device)
        map_known_indice = torch.cat([torch.arange(n, device=device) for n in known_num])
        map_known_indice = torch.cat([map_known_indice + dn_single_pad * i for i in range(groups)]).long()
        dn_query_bbox = dn_query_bbox.index_put((known_bid, map_known_indice), known_bbox_expand)
        dn_query_feat = dn_query_feat.index_put((known_bid, map_known_indice), known_feat_expand)
        input_query_bbox = torch.cat([dn_query_bbox, init_query_bbox], dim=1)
        input_query_feat = torch.cat([dn_query_feat, init_query_feat], dim=1)

        # key j is blocked for query i iff j is a denoising query of another group than i's (the matching queries are in none)
        idx = torch.arange(dn_pad_size + Q, device=device)
        group = torch.where(idx < dn_pad_size, torch.div(idx, dn_single_pad, rounding_mode="floor"), torch.full_like(idx, -1))
        attn_mask = (idx[None, :] < dn_pad_size) & (group[:, None] != group[None, :])
        mask_dict = {"known_indice": known_indice, "batch_idx": batch_idx, "map_known_indice": map_known_indice,
                     "known_lbs_bboxes": (known_labels, known_bboxs), "pad_size": dn_pad_size}
        return input_query_bbox, input_query_feat, attn_mask, mask_dict

    def prepare_for_dn_loss(self, mask_dict):
        """racformer_head.py:249-262: the denoising outputs gathered per ground-truth copy, [layers, groups*n, .] -- pure
        indexing, the input of the denoising loss."""
        cls_scores, bbox_preds = mask_dict["output_known_lbs_bboxes"]
        known_labels, known_bboxs = mask_dict["known_lbs_bboxes"]
        map_known_indice = mask_dict["map_known_indice"].long()
        known_indice = mask_dict["known_indice"].long()
        bid = mask_dict["batch_idx"].long()[known_indice]
        num_tgt = known_indice.numel()
        if len(cls_scores) > 0:
            cls_scores = cls_scores.permute(1, 2, 0, 3)[(bid, map_known_indice)].permute(1, 0, 2)
            bbox_preds = bbox_preds.permute(1, 2, 0, 3)[(bid, map_known_indice)].permute(1, 0, 2)
        return known_labels, known_bboxs, cls_scores, bbox_preds, num_tgt

    # ------------------------------------------------------------------------------------------------ losses
    def _require_losses(self):
        if self.assigner is None or self.loss_cls is None or self.loss_bbox is None:
            raise NotImplementedError("racformer_amd: assigner and losses are not built")

    def _avg_factors(self, num_total_pos, like):
        """(cls_avg_factor, box avg factor) of loss_single (:396-409): host numbers outside torch.distributed, 0-dim device
        tensors under it (the all_reduce stays on the stream)"""
        cls_avg = num_total_pos * 1.0
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            mean = reduce_mean(like.new_tensor([cls_avg]))[0]
            return (mean.clamp(min=1) if self.sync_cls_avg_factor else max(cls_avg, 1)), mean.clamp(min=1)
        return max(cls_avg, 1), max(cls_avg, 1.0)

    def dn_loss_single(self, cls_scores, bbox_preds, known_bboxs, known_labels, num_total_pos=None):
        """racformer_head.py:264-300"""
        num_total_pos = self._avg_factors(num_total_pos, cls_scores)[1]
        cls_scores = cls_scores.reshape(-1, self.cls_out_channels)
        bbox_weights = torch.ones_like(bbox_preds)
        label_weights = torch.ones_like(known_labels)
        loss_cls = self.loss_cls(cls_scores, known_labels.long(), label_weights, avg_factor=num_total_pos)
        bbox_preds = bbox_preds.reshape(-1, bbox_preds.size(-1))
        normalized_bbox_targets = normalize_bbox(known_bboxs)
        isnotnan = torch.isfinite(normalized_bbox_targets).all(dim=-1)
        bbox_weights = bbox_weights * self.code_weights
        loss_bbox = self.loss_bbox(bbox_preds[isnotnan, :10], normalized_bbox_targets[isnotnan, :10], bbox_weights[isnotnan, :10],
                                   avg_factor=num_total_pos)
        return self.dn_weight * torch.nan_to_num(loss_cls), self.dn_weight * torch.nan_to_num(loss_bbox)

    def calc_dn_loss(self, loss_dict, preds_dicts, num_dec_layers):
        """racformer_head.py:302-324"""
        known_labels, known_bboxs, cls_scores, bbox_preds, num_tgt = self.prepare_for_dn_loss(preds_dicts["dn_mask_dict"])
        dn_losses_cls, dn_losses_bbox = multi_apply(self.dn_loss_single, cls_scores, bbox_preds, [known_bboxs] * num_dec_layers,
                                                    [known_labels] * num_dec_layers, [num_tgt] * num_dec_layers)
        return self._fill_loss_dict(loss_dict, dn_losses_cls, dn_losses_bbox, "_dn")

    @staticmethod
    def _fill_loss_dict(loss_dict, losses_cls, losses_bbox, suffix=""):
        """the last layer under the plain keys, layer i before it under 'd{i}.' (:315-322, :476-484)"""
        loss_dict["loss_cls" + suffix], loss_dict["loss_bbox" + suffix] = losses_cls[-1], losses_bbox[-1]
        for i, (c, b) in enumerate(zip(losses_cls[:-1], losses_bbox[:-1])):
            loss_dict[f"d{i}.loss_cls" + suffix], loss_dict[f"d{i}.loss_bbox" + suffix] = c, b
        return loss_dict

    def _get_target_single(self, cls_score, bbox_pred, gt_labels, gt_bboxes, gt_bboxes_ignore=None):
        """racformer_head.py:326-352 (the pseudo sampler: the positive rows are the assigned ones)"""
        num_bboxes = bbox_pred.size(0)
        assigned_gt_inds, _ = self.assigner.assign(bbox_pred, cls_score, gt_bboxes, gt_labels, gt_bboxes_ignore, self.code_weights, True)
        pos_inds = torch.nonzero(assigned_gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg_inds = torch.nonzero(assigned_gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        pos_assigned_gt_inds = assigned_gt_inds[pos_inds] - 1
        labels = gt_bboxes.new_full((num_bboxes,), self.num_classes, dtype=torch.long)
        labels[pos_inds] = gt_labels.long()[pos_assigned_gt_inds]
        label_weights = gt_bboxes.new_ones(num_bboxes)
        bbox_targets = torch.zeros_like(bbox_pred)[..., :9]
        bbox_weights = torch.zeros_like(bbox_pred)
        bbox_weights[pos_inds] = 1.0
        bbox_targets[pos_inds] = gt_bboxes[pos_assigned_gt_inds].to(bbox_targets.dtype)
        return labels, label_weights, bbox_targets, bbox_weights, pos_inds, neg_inds

    def get_targets(self, cls_scores_list, bbox_preds_list, gt_bboxes_list, gt_labels_list, gt_bboxes_ignore_list=None):
        """racformer_head.py:354-372"""
        assert gt_bboxes_ignore_list is None, "Only supports for gt_bboxes_ignore setting to None."
        ignore = [None] * len(cls_scores_list)
        labels, label_weights, bbox_targets, bbox_weights, pos, neg = multi_apply(
            self._get_target_single, cls_scores_list, bbox_preds_list, gt_labels_list, gt_bboxes_list, ignore)
        return labels, label_weights, bbox_targets, bbox_weights, sum(i.numel() for i in pos), sum(i.numel() for i in neg)

    def loss_single(self, cls_scores, bbox_preds, gt_bboxes_list, gt_labels_list, gt_bboxes_ignore_list=None):
        """racformer_head.py:374-427: one decoder layer, [B,Q,.] outputs"""
        num_imgs = cls_scores.size(0)
        labels_list, label_weights_list, bbox_targets_list, bbox_weights_list, num_total_pos, num_total_neg = self.get_targets(
            [cls_scores[i] for i in range(num_imgs)], [bbox_preds[i] for i in range(num_imgs)], gt_bboxes_list, gt_labels_list,
            gt_bboxes_ignore_list)
        labels, label_weights = torch.cat(labels_list, 0), torch.cat(label_weights_list, 0)
        bbox_targets, bbox_weights = torch.cat(bbox_targets_list, 0), torch.cat(bbox_weights_list, 0)
        cls_scores = cls_scores.reshape(-1, self.cls_out_channels)
        cls_avg_factor, box_avg_factor = self._avg_factors(num_total_pos * 1.0 + num_total_neg * self.bg_cls_weight, cls_scores)
        loss_cls = self.loss_cls(cls_scores, labels, label_weights, avg_factor=cls_avg_factor)
        bbox_preds = bbox_preds.reshape(-1, bbox_preds.size(-1))
        normalized_bbox_targets = normalize_bbox(bbox_targets)
        isnotnan = torch.isfinite(normalized_bbox_targets).all(dim=-1)
        bbox_weights = bbox_weights * self.code_weights
        loss_bbox = self.loss_bbox(bbox_preds[isnotnan, :10], normalized_bbox_targets[isnotnan, :10], bbox_weights[isnotnan, :10],
                                   avg_factor=box_avg_factor)
        return torch.nan_to_num(loss_cls), torch.nan_to_num(loss_bbox)

    def _loss_inputs(self, gt_bboxes_list, gt_labels_list, preds_dicts, gt_bboxes_ignore):
        assert gt_bboxes_ignore is None, f"{self.__class__.__name__} only supports for gt_bboxes_ignore setting to None."
        if preds_dicts.get("enc_cls_scores") is not None:
            raise NotImplementedError("racformer_amd: encoder proposals (enc_cls_scores) have no loss here; the head never emits them")
        all_cls_scores, all_bbox_preds = preds_dicts["all_cls_scores"], preds_dicts["all_bbox_preds"]
        device = all_cls_scores.device
        gt_bboxes_list = [plain_gt_boxes(gt, device) for gt in gt_bboxes_list]
        gt_labels_list = [lab.to(device) for lab in gt_labels_list]
        return all_cls_scores, all_bbox_preds, gt_bboxes_list, gt_labels_list

    def loss_unfused(self, gt_bboxes_list, gt_labels_list, preds_dicts, gt_bboxes_ignore=None):
        """racformer_head.py:429-485 as the reference runs it: per layer and per sample a torch cost matrix, a copy to the host,
        the host solver, scattered targets, FocalLoss and L1Loss.  Any device and dtype; the comparison of the fused route."""
        self._require_losses()
        all_cls_scores, all_bbox_preds, gt_bboxes_list, gt_labels_list = self._loss_inputs(gt_bboxes_list, gt_labels_list, preds_dicts,
                                                                                           gt_bboxes_ignore)
        num_dec_layers = len(all_cls_scores)
        losses_cls, losses_bbox = multi_apply(self.loss_single, all_cls_scores, all_bbox_preds, [gt_bboxes_list] * num_dec_layers,
                                              [gt_labels_list] * num_dec_layers, [None] * num_dec_layers)
        loss_dict = dict()
        if preds_dicts.get("dn_mask_dict") is not None:
            loss_dict = self.calc_dn_loss(loss_dict, preds_dicts, num_dec_layers)
        return self._fill_loss_dict(loss_dict, losses_cls, losses_bbox)

    def _fused_loss_applies(self, all_cls_scores, all_bbox_preds, counts):
        Q = all_cls_scores.shape[2]
        return all_cls_scores.is_cuda and all_cls_scores.dtype == torch.float32 and all_bbox_preds.dtype == torch.float32 \
            and all_bbox_preds.shape[-1] == 10 and self.assigner.fusable() and type(self.loss_cls) is FocalLoss \
            and type(self.loss_bbox) is L1Loss and Q <= 2048 and max(counts, default=0) <= Q and len(counts) <= 64

    def loss(self, gt_bboxes_list, gt_labels_list, preds_dicts, gt_bboxes_ignore=None):
        """racformer_head.py:429-485 -> {'loss_cls', 'loss_bbox', 'd{i}.loss_cls', 'd{i}.loss_bbox'} and, with denoising queries,
        the same keys with '_dn'.  gt_bboxes_list: per sample an object with ``.gravity_center`` and ``.tensor`` or a plain [n,9]
        tensor; gt_labels_list: integer tensors.

        CUDA float32 outputs take the fused route: rac_match_cost_fwd, rac_lsap_fwd and rac_det_loss_fwd once for all layers and
        samples, rac_det_loss_fwd once more for the denoising rows -- no read-back to the host (the counts of positives are the
        lengths of the ground-truth lists).  Everything else (CPU, other dtypes, a sample with more boxes than queries, more than
        2048 queries) takes loss_unfused."""
        self._require_losses()
        all_cls_scores, all_bbox_preds, gt_bboxes_list, gt_labels_list = self._loss_inputs(gt_bboxes_list, gt_labels_list, preds_dicts,
                                                                                           gt_bboxes_ignore)
        counts = [int(g.shape[0]) for g in gt_bboxes_list]
        if not self._fused_loss_applies(all_cls_scores, all_bbox_preds, counts):
            return self.loss_unfused(gt_bboxes_list, gt_labels_list, preds_dicts)
        from .fused import lsap_fused, match_cost_fused
        L, B, Q, C = all_cls_scores.shape
        cls, box = all_cls_scores.contiguous(), all_bbox_preds.contiguous()
        table = torch.cat(gt_bboxes_list).float().contiguous()
        labels = torch.cat(gt_labels_list).to(torch.int32)
        code_weights = self.code_weights.detach().float().contiguous()
        a = self.assigner
        if max(counts) > 0:
            cost = match_cost_fused(cls.detach(), box.detach(), table, labels, counts, code_weights, a.cls_cost.weight, a.reg_cost.weight,
                                    a.theta_cost.weight if a.polar else None)
            assigned = lsap_fused(cost, counts, L, Q)[1]
        else:
            assigned = torch.full((L * B, Q), -1, device=cls.device, dtype=torch.int32)
        alpha, gamma = self.loss_cls.alpha, self.loss_cls.gamma
        sums = head_loss_sums(cls.view(L, B * Q, C), box.view(L, B * Q, 10), assigned.view(L, B * Q), table, labels, code_weights, alpha, gamma)
        num_total_pos = sum(min(Q, n) for n in counts)
        cls_avg, box_avg = self._avg_factors(num_total_pos * 1.0 + (B * Q - num_total_pos) * self.bg_cls_weight, cls)
        losses_cls = torch.nan_to_num(self.loss_cls.loss_weight * (sums[:, 0] / (cls_avg + _EPS32)))
        losses_bbox = torch.nan_to_num(self.loss_bbox.loss_weight * (sums[:, 1] / (box_avg + _EPS32)))
        loss_dict = dict()
        md = preds_dicts.get("dn_mask_dict")
        if md is not None:
            known_labels, known_bboxs, dn_cls, dn_box, num_tgt = self.prepare_for_dn_loss(md)
            total = int(md["batch_idx"].numel())                # row r of a layer belongs to box r mod total (:180-183)
            dn_sums = head_loss_sums(dn_cls, dn_box, None, known_bboxs[:total].float().contiguous(), known_labels[:total].to(torch.int32),
                                     code_weights, alpha, gamma)
            dn_avg = self._avg_factors(num_tgt, cls)[1]
            dn_cls_l = self.dn_weight * torch.nan_to_num(self.loss_cls.loss_weight * (dn_sums[:, 0] / (dn_avg + _EPS32)))
            dn_box_l = self.dn_weight * torch.nan_to_num(self.loss_bbox.loss_weight * (dn_sums[:, 1] / (dn_avg + _EPS32)))
            self._fill_loss_dict(loss_dict, dn_cls_l.unbind(0), dn_box_l.unbind(0), "_dn")
        return self._fill_loss_dict(loss_dict, losses_cls.unbind(0), losses_bbox.unbind(0))

    def get_bboxes(self, preds_dicts, img_metas, rescale=False):
        """racformer_head.py:488-507 (VERSION 'v1.0.0').  Boxes are returned as a plain [n,9] tensor
        (x, y, z_bottom, w, l, h, yaw, vx, vy) -- mmdet3d's LiDARInstance3DBoxes wrapper is not a
        dependency here."""
        ret_list = []
        for preds in self.bbox_coder.decode(preds_dicts):
            bboxes = preds["bboxes"]
            bboxes = torch.cat([bboxes[:, :2], bboxes[:, 2:3] - bboxes[:, 5:6] * 0.5, bboxes[:, 3:]], dim=1)
            ret_list.append([bboxes, preds["scores"], preds["labels"]])
        return ret_list

    def get_detections_fixed(self, preds_dicts):
        """Shape-static detections for the data-parallel all-gather: [B, max_num, 11] =
        (9 box dims with z at the box bottom, score, label); rows that fail the centre-range /
        score masks carry score = -1.  Same numbers as get_bboxes, no host synchronisation."""
        cls, box = preds_dicts["all_cls_scores"][-1], preds_dicts["all_bbox_preds"][-1]
        coder = self.bbox_coder
        if cls.is_cuda and cls.dtype == torch.float32 and cls.shape[1] * cls.shape[2] <= 16384 and coder.max_num <= 512 \
                and coder.post_center_range is not None and box.shape[-1] == 10:
            # one HIP launch per sample (rac_decode_fwd) instead of ~15 torch launches
            from .fused import decode_fused
            res = torch.empty(cls.size(0), coder.max_num, 11, device=cls.device, dtype=torch.float32)
            for i in range(cls.size(0)):
                decode_fused(cls[i], box[i], coder.max_num, coder.post_center_range, coder.score_threshold, out=res[i])
            return res
        out = []
        for i in range(cls.size(0)):
            b, s, l, keep = self.bbox_coder.topk_fixed(cls[i], box[i])
            b = torch.cat([b[:, :2], b[:, 2:3] - b[:, 5:6] * 0.5, b[:, 3:]], dim=1)
            s = torch.where(keep, s, torch.full_like(s, -1.0))
            out.append(torch.cat([b, s[:, None], l[:, None].to(b.dtype)], dim=1))
        return torch.stack(out)
