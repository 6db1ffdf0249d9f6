"""Counterparts of ``RaCFormer_head`` (models/racformer_head.py:13-262, 488-507)
and ``NMSFreeCoder`` (models/bbox/coders/nms_free_coder.py:8-110): same names, constructor
arguments, ``forward`` / ``get_bboxes`` / ``decode`` behaviour and ``state_dict`` keys
(``init_query_bbox.weight``, ``label_enc.weight``, ``code_weights``, ``transformer.*``).
Training mode builds the query-denoising inputs (``prepare_for_dn_input``), runs the decoder under their attention mask and
returns the reference's dict with ``dn_mask_dict``; ``prepare_for_dn_loss`` is there for the losses.  The assigner and the losses
themselves are not built: ``loss`` raises."""
import math

import torch
import torch.nn as nn

from .bbox_utils import const_tensor, denormalize_bbox, encode_bbox, xy2theta_d_coods
from .transformer import RaCFormerTransformer


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
    """models/racformer_head.py without the assigner and the losses.  ``transformer`` is a config dict
    (``type='RaCFormerTransformer'``, as in configs/racformer_r50_nuimg_704x256_f8.py:152-166) or a
    module; ``bbox_coder`` a config dict (``type='NMSFreeCoder'``) or an instance."""

    def __init__(self, *args, num_classes, in_channels, num_query=900, num_clusters=5, transformer=None,
                 bbox_coder=None, code_size=10, code_weights=[1.0] * 10, query_denoising=True,
                 query_denoising_groups=10, train_cfg=dict(), test_cfg=dict(max_per_img=100), **kwargs):
        super().__init__()
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

    def forward(self, mlvl_feats, lss_bev_feats, radar_bev_feats, img_metas):
        """racformer_head.py:82-134.  Eval mode: the eval branch of prepare_for_dn_input (:142-145, :241-245) with cached initial
        queries and the fused output tail.  Training mode: forward_training."""
        if self.training:
            return self.forward_training(mlvl_feats, lss_bev_feats, radar_bev_feats, img_metas)
        B = lss_bev_feats.shape[0]
        Q = self.num_query
        # the initial queries depend on the embeddings only: built once per (weights, batch size) in eval, not per forward
        # (four small launches per step otherwise); the decoder never writes into its inputs
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
        pc = self.pc_range
        if lss_bev_feats.is_cuda and self.code_size == 10 and not torch.is_grad_enabled():
            # nan_to_num of both outputs, the centre's scaling to metres and the column reorder: one HIP launch instead of five
            from .fused import head_finish_fused
            cls_scores, bbox_xy = self.transformer(query_bbox, query_feat, mlvl_feats, lss_bev_feats, radar_bev_feats,
                                                   attn_mask=None, img_metas=img_metas, raw=True)
            if cls_scores.dtype == torch.float32 and bbox_xy.dtype == torch.float32:
                cls_scores, bbox_preds = head_finish_fused(cls_scores.contiguous(), bbox_xy.contiguous(), pc)
                return {"all_cls_scores": cls_scores, "all_bbox_preds": bbox_preds, "enc_cls_scores": None, "enc_bbox_preds": None}
            cls_scores, bbox_preds = torch.nan_to_num(cls_scores), torch.nan_to_num(bbox_xy)
        else:
            cls_scores, bbox_preds = self.transformer(query_bbox, query_feat, mlvl_feats, lss_bev_feats,
                                                      radar_bev_feats, attn_mask=None, img_metas=img_metas)
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

    def loss(self, *args, **kwargs):
        raise NotImplementedError("racformer_amd: assigner and losses are not built")

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
