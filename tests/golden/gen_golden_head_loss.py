#!/usr/bin/env python3
"""Golden head losses: runs the REFERENCE's own RaCFormer_head.loss (racformer_head.py:429-485) with the f8 config's loss and
assigner dicts (configs/racformer_r50_nuimg_704x256_f8.py:150, 180-199) and code_weights [2,2,1,...] on CPU, in float32 and
float64, and writes a data-only fixture next to this script.  Build container only (reference tree + scipy, see
ref_loader_loss.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_head_loss.py

  head_loss_small.npz   L = 2 layers, 10 classes, 3 denoising groups.  Cases (keys prefixed "a:" / "b:" / "c:"):
     a   Q = 70,  B = 2, G = (5, 0)
     b   Q = 70,  B = 2, G = (65, 1); the single box of sample 1 has w = 0 (a non-finite target: its cost row is 100 everywhere)
     c   Q = 130, B = 2, G = (3, 40); sample 0 is one box three times; layer 0 / sample 0 has one NaN and one +inf logit in the
         class of that box
     per case: all_cls_scores, all_bbox_preds [L,B,Q,.], dn_cls, dn_box [L,B,pad,.] (the decoder's denoising outputs, drawn), the
     mask_dict entries of the reference's prepare_for_dn_input, gt_boxes{b} / gt_labels{b}; per problem (l, b) with boxes:
     cost32:{l}:{b} / cost64:{l}:{b} [Q,G] as scipy saw them, rows / cols (scipy's assignment on the float32 cost), total64,
     margin; the loss dict as loss32:<key> / loss64:<key>; gradients of sum(losses) w.r.t. the four leaves as grad32:<leaf> /
     grad64:<leaf>.

Every recorded assignment is the UNIQUE optimum by a margin: for each matched pair, that pair is forbidden, the problem re-solved
with scipy, and the smallest increase of the total cost is the problem's margin; the generator asserts margin >= 1e-3 (else it
draws the next seed) and that the float64 run found the same assignment.  Exempt are the two problems that are degenerate by
construction -- the repeated box (c, sample 0) and the constant row of the w = 0 box (b, sample 1): margin is recorded as 0 there
and tests check total cost and certificate only.  Ground-truth centres cover all four quadrants (the theta wrap)."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_loader_loss  # noqa: E402
import ref_loader  # noqa: E402
from scipy.optimize import linear_sum_assignment  # noqa: E402

L, NUM_CLASSES, GROUPS, EMBED, NUM_CLUSTERS = 2, 10, 3, 32, 5
PC_RANGE = [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]
POST_RANGE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]
CODE_WEIGHTS = [2.0, 2.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
LOSS_CLS = dict(type="FocalLoss", use_sigmoid=True, gamma=2.0, alpha=0.25, loss_weight=2.0)
LOSS_BBOX = dict(type="L1Loss", loss_weight=0.25)
LOSS_IOU = dict(type="GIoULoss", loss_weight=0.0)
ASSIGNER = dict(type="PolarHungarianAssigner3D", cls_cost=dict(type="FocalLossCost", weight=2.0),
                reg_cost=dict(type="BBox3DL1Cost", weight=0.25), theta_cost=dict(type="ThetaL1Cost", weight=3.0),
                iou_cost=dict(type="IoUCost", weight=0.0))
CASES = {"a": dict(Q=70, G=(5, 0)), "b": dict(Q=70, G=(65, 1)), "c": dict(Q=130, G=(3, 40))}
MARGIN = 1e-3
LEAVES = ("all_cls_scores", "all_bbox_preds", "dn_cls", "dn_box")


def make_gt(rng, n):
    box = np.zeros((n, 9), np.float32)
    quad = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1]], np.float32)[np.arange(n) % 4]       # all four quadrants
    box[:, 0:2] = rng.uniform(3.0, 48.0, (n, 2)) * quad
    box[:, 2] = rng.uniform(-2.0, 1.0, n)
    box[:, 3:6] = rng.uniform(0.5, 5.0, (n, 3))
    box[:, 6] = rng.uniform(-np.pi, np.pi, n)
    box[:, 7:9] = rng.uniform(-3.0, 3.0, (n, 2))
    return box, rng.integers(0, NUM_CLASSES, n).astype(np.int64)


def make_preds(rng, B, Q):
    """decoder outputs in the head's output format: (cx, cy [m], log w, log l, cz [m], log h, sin, cos, vx, vy)"""
    cls = rng.normal(-2.0, 1.5, (L, B, Q, NUM_CLASSES)).astype(np.float32)
    box = np.zeros((L, B, Q, 10), np.float32)
    box[..., 0:2] = rng.uniform(-50.0, 50.0, (L, B, Q, 2))
    box[..., 2:4] = rng.uniform(-0.7, 1.7, (L, B, Q, 2))
    box[..., 4] = rng.uniform(-2.0, 1.0, (L, B, Q))
    box[..., 5] = rng.uniform(-0.7, 1.7, (L, B, Q))
    ang = rng.uniform(-np.pi, np.pi, (L, B, Q))
    box[..., 6], box[..., 7] = np.sin(ang), np.cos(ang)
    box[..., 8:10] = rng.uniform(-3.0, 3.0, (L, B, Q, 2))
    return cls, box


def build_head(ref, Q):
    ref_loader._TRANSFORMER.classes["_NoTransformer"] = lambda **k: types.SimpleNamespace(embed_dims=EMBED)
    torch.manual_seed(1)
    head = ref.racformer_head.RaCFormer_head(
        num_classes=NUM_CLASSES, in_channels=EMBED, num_query=Q, num_clusters=NUM_CLUSTERS, code_size=10, code_weights=CODE_WEIGHTS,
        query_denoising=True, query_denoising_groups=GROUPS, sync_cls_avg_factor=True, transformer=dict(type="_NoTransformer"),
        bbox_coder=dict(type="NMSFreeCoder", post_center_range=POST_RANGE, pc_range=PC_RANGE, max_num=20, score_threshold=0.05,
                        num_classes=NUM_CLASSES),
        loss_cls=LOSS_CLS, loss_bbox=LOSS_BBOX, loss_iou=LOSS_IOU, train_cfg=dict(assigner=ASSIGNER))
    head.training = True
    return head


def margin_of(cost, rows, cols):
    total = cost[rows, cols].sum()
    inc = []
    for r, c in zip(rows, cols):
        forbidden = cost.copy()
        forbidden[r, c] = 1e6
        rr, cc = linear_sum_assignment(forbidden)
        inc.append(forbidden[rr, cc].sum() - total)
    return float(min(inc))


def run_case(ref, name, spec, seed):
    """-> dict of arrays, or None if a margin is too small"""
    rng = np.random.default_rng(seed)
    Q, counts = spec["Q"], spec["G"]
    B = len(counts)
    head = build_head(ref, Q)
    d = {"seed": np.array(seed), "Q": np.array(Q), "counts": np.array(counts)}
    gts = []
    for b, n in enumerate(counts):
        box, lab = make_gt(rng, n)
        if name == "b" and b == 1:
            box[0, 3] = 0.0                                             # w = 0: log w = -inf
        if name == "c" and b == 0:
            box[:], lab[:] = box[0], lab[0]                             # one box, three times
        d[f"gt_boxes{b}"], d[f"gt_labels{b}"] = box, lab
        gts.append((box, lab))
    cls, box = make_preds(rng, B, Q)
    if name == "c":
        k = int(gts[0][1][0])
        cls[0, 0, 7, k], cls[0, 0, 19, k] = np.nan, np.inf
    # the denoising part: the reference's own prepare_for_dn_input for the index tensors, drawn decoder outputs for its rows
    metas = [{"gt_bboxes_3d": types.SimpleNamespace(gravity_center=torch.from_numpy(g[:, :3]), tensor=torch.from_numpy(g)),
              "gt_labels_3d": torch.from_numpy(lab)} for g, lab in gts]
    torch.manual_seed(seed)
    init = head.init_query_bbox.weight.detach().clone().view(1, Q, 10).repeat(B, 1, 1)
    with torch.no_grad():
        _, _, _, md = head.prepare_for_dn_input(B, init, head.label_enc, metas)
    pad = int(md["pad_size"])
    dn_cls, dn_box = make_preds(rng, B, pad)
    d.update(all_cls_scores=cls, all_bbox_preds=box, dn_cls=dn_cls, dn_box=dn_box, pad_size=np.array(pad),
             known_indice=md["known_indice"].numpy(), batch_idx=md["batch_idx"].numpy(), map_known_indice=md["map_known_indice"].numpy(),
             known_labels=md["known_lbs_bboxes"][0].numpy(), known_bboxs=md["known_lbs_bboxes"][1].numpy())

    mod = ref.polar_hungarian_assigner_3d
    solved = {}
    for dtype, tag in ((torch.float32, "32"), (torch.float64, "64")):
        seen = []

        def recorder(cost):
            c = cost.numpy().copy()
            r, cc = linear_sum_assignment(c)
            seen.append((c, r, cc))
            return r, cc
        mod.linear_sum_assignment = recorder
        head = head.to(dtype)
        leaves = {k: torch.from_numpy(d[k]).to(dtype).requires_grad_() for k in LEAVES}
        mask_dict = {"known_indice": md["known_indice"], "batch_idx": md["batch_idx"], "map_known_indice": md["map_known_indice"],
                     "known_lbs_bboxes": (md["known_lbs_bboxes"][0], md["known_lbs_bboxes"][1].to(dtype)), "pad_size": pad,
                     "output_known_lbs_bboxes": (leaves["dn_cls"], leaves["dn_box"])}
        preds = {"all_cls_scores": leaves["all_cls_scores"], "all_bbox_preds": leaves["all_bbox_preds"], "enc_cls_scores": None,
                 "enc_bbox_preds": None, "dn_mask_dict": mask_dict}
        gt_boxes = [types.SimpleNamespace(gravity_center=torch.from_numpy(g[:, :3]).to(dtype), tensor=torch.from_numpy(g).to(dtype))
                    for g, _ in gts]
        losses = head.loss(gt_boxes, [torch.from_numpy(lab) for _, lab in gts], preds)
        sum(losses.values()).backward()
        for k, v in losses.items():
            d[f"loss{tag}:{k}"] = v.detach().numpy()
        for k, v in leaves.items():
            d[f"grad{tag}:{k}"] = v.grad.numpy()
        # the assigner ran once per (layer, sample with boxes), layers outermost
        problems = [(l, b) for l in range(L) for b in range(B) if counts[b] > 0]
        assert len(seen) == len(problems)
        for (l, b), (c, r, cc) in zip(problems, seen):
            d[f"cost{tag}:{l}:{b}"] = c
            solved[(tag, l, b)] = (c, r, cc)
    for (tag, l, b), (c, r, cc) in solved.items():
        if tag != "32":
            continue
        degenerate = (name == "b" and b == 1) or (name == "c" and b == 0)
        c64, r64, cc64 = solved[("64", l, b)]
        d[f"rows:{l}:{b}"], d[f"cols:{l}:{b}"] = r.astype(np.int64), cc.astype(np.int64)
        d[f"total64:{l}:{b}"] = np.array(c.astype(np.float64)[r, cc].sum())
        if degenerate:
            d[f"margin:{l}:{b}"] = np.array(0.0)
            continue
        m = min(margin_of(c.astype(np.float64), r, cc), margin_of(c64, r64, cc64))
        if m < MARGIN or not (np.array_equal(r, r64) and np.array_equal(cc, cc64)):
            print(f"  case {name} seed {seed}: problem ({l},{b}) has margin {m:.2e}; next seed")
            return None
        d[f"margin:{l}:{b}"] = np.array(m)
    return d


def main():
    ref = ref_loader_loss.load_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self          # this process only: the reference's .cuda() on a CPU-only machine
    out = {"code_weights": np.array(CODE_WEIGHTS, np.float32), "num_layers": np.array(L), "groups": np.array(GROUPS)}
    for name, spec in CASES.items():
        seed = 100 * (ord(name) - ord("a") + 1)
        while True:
            d = run_case(ref, name, spec, seed)
            if d is not None:
                break
            seed += 1
        out.update({f"{name}:{k}": v for k, v in d.items()})
        margins = {k: float(v) for k, v in d.items() if k.startswith("margin:")}
        print(f"  case {name}: seed {seed}, pad {int(d['pad_size'])}, margins {margins}")
        print("   ", {k[7:]: float(np.ravel(v)[0]) for k, v in d.items() if k.startswith("loss32:")})
    path = os.path.join(HERE, "head_loss_small.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote head_loss_small.npz: {os.path.getsize(path) / 1024:.1f} KiB, {len(out)} arrays")


if __name__ == "__main__":
    main()
