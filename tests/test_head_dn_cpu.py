"""RaCFormer_head's query denoising without a GPU: prepare_for_dn_input against the reference's own
(tests/golden/dn_input_small.npz, gen_golden_dn_input.py) bit for bit under the same seed, the mask against its closed form,
prepare_for_dn_loss, ``loss``, and the head's forward in training mode on the tiny rig of tests/test_decoder_grad_cpu.py with
the HIP launchers replaced by fakes (the two SASA launchers by the float64 masked fakes of tests/sasa_mask_ref.py)."""
import os
import types

import numpy as np
import pytest
import torch

import sasa_mask_ref as MR
import test_decoder_grad_cpu as DG
from test_decoder_grad_cpu import fakes  # noqa: F401  (the fixture)
from racformer_amd import synthetic as syn
from racformer_amd import transformer as T
from racformer_amd.fused import PackedAttnMask
from racformer_amd.head import RaCFormer_head

CFG = syn.SMALL6
POST_RANGE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]


def t(a):
    return torch.from_numpy(np.asarray(a)).clone()


def small_head(g):
    """the generator's head: 20 queries in 4 clusters, 10 classes, 3 groups, embed_dims 32 -- no transformer"""
    head = RaCFormer_head(num_classes=10, in_channels=32, num_query=20, num_clusters=4, code_size=10, query_denoising=True,
                          query_denoising_groups=3, transformer=None,
                          bbox_coder=dict(type="NMSFreeCoder", post_center_range=POST_RANGE, pc_range=list(syn.PC_RANGE), max_num=20,
                                          score_threshold=0.05, num_classes=10))
    with torch.no_grad():
        head.init_query_bbox.weight.copy_(t(g["init_query_bbox"]))
        head.label_enc.weight.copy_(t(g["label_enc"]))
    return head.train()


def metas_of(g, case, boxes_as):
    metas, i = [], 0
    while f"{case}:gt_boxes{i}" in g:
        box = t(g[f"{case}:gt_boxes{i}"])
        gt = box if boxes_as == "tensor" else types.SimpleNamespace(gravity_center=box[:, :3], tensor=box)
        metas.append({"gt_bboxes_3d": gt, "gt_labels_3d": t(g[f"{case}:gt_labels{i}"])})
        i += 1
    return metas


@pytest.mark.parametrize("boxes_as", ["tensor", "object"])
@pytest.mark.parametrize("case", ["a", "b"])
def test_prepare_for_dn_input_reproduces_the_reference(golden_dir, case, boxes_as):
    g = np.load(os.path.join(golden_dir, "dn_input_small.npz"))
    head = small_head(g)
    assert (head.dn_enabled, head.dn_group_num, head.dn_weight, head.dn_bbox_noise_scale, head.dn_label_noise_scale) == (True, 3, 1.0, 0.5, 0.5)
    metas = metas_of(g, case, boxes_as)
    B = len(metas)
    init = head.init_query_bbox.weight.detach().clone().view(1, 20, 10).repeat(B, 1, 1)
    torch.manual_seed(int(g[f"{case}:seed"]))
    with torch.no_grad():
        qb, qf, mask, md = head.prepare_for_dn_input(B, init, head.label_enc, metas)
    assert torch.equal(qb, t(g[f"{case}:input_query_bbox"]))
    assert torch.equal(qf, t(g[f"{case}:input_query_feat"]))
    assert mask.dtype == torch.bool and torch.equal(mask, t(g[f"{case}:attn_mask"]))
    assert md["pad_size"] == int(g[f"{case}:pad_size"]) == 3 * max(m["gt_labels_3d"].numel() for m in metas)
    for key in ("known_indice", "batch_idx", "map_known_indice"):
        assert md[key].dtype == torch.int64 and torch.equal(md[key], t(g[f"{case}:{key}"])), key
    assert torch.equal(md["known_lbs_bboxes"][0], t(g[f"{case}:known_labels"]))
    assert torch.equal(md["known_lbs_bboxes"][1], t(g[f"{case}:known_bboxs"]))
    # the mask's closed form: key j is allowed for query i iff j is a matching query or j is in i's group
    pad, single = md["pad_size"], md["pad_size"] // 3
    Q = pad + 20
    for i in range(Q):
        for j in range(Q):
            allowed = j >= pad or (i < pad and i // single == j // single)
            assert bool(mask[i, j]) == (not allowed), (i, j)
    assert torch.equal(mask, MR.dn_layout(Q, 3, single))


def test_prepare_for_dn_input_without_boxes_and_outside_training(golden_dir):
    g = np.load(os.path.join(golden_dir, "dn_input_small.npz"))
    head = small_head(g)
    init = head.init_query_bbox.weight.detach().clone().view(1, 20, 10).repeat(2, 1, 1)
    empty = [{"gt_bboxes_3d": torch.zeros(0, 9), "gt_labels_3d": torch.zeros(0, dtype=torch.long)}] * 2
    qb, qf, mask, md = head.prepare_for_dn_input(2, init, head.label_enc, empty)
    assert qb is init and tuple(qf.shape) == (2, 20, 32) and mask is None and md["pad_size"] == 0
    plain = torch.cat([head.label_enc.weight[10].repeat(20, 1), torch.zeros(20, 1)], dim=1)
    assert torch.equal(qf[0], plain) and torch.equal(qf[1], plain)
    for h in (head.eval(), small_head(g)):
        if h.training:
            h.dn_enabled = False
        qb, qf2, mask, md = h.prepare_for_dn_input(2, init, h.label_enc, metas_of(g, "a", "tensor"))
        assert qb is init and torch.equal(qf2, qf) and mask is None and md is None


def test_prepare_for_dn_loss_is_the_references_indexing(golden_dir):
    g = np.load(os.path.join(golden_dir, "dn_input_small.npz"))
    head = small_head(g)
    metas = metas_of(g, "a", "tensor")
    init = head.init_query_bbox.weight.detach().clone().view(1, 20, 10).repeat(2, 1, 1)
    torch.manual_seed(3)
    _, _, _, md = head.prepare_for_dn_input(2, init, head.label_enc, metas)
    L, pad = 6, md["pad_size"]
    gen = torch.Generator().manual_seed(5)
    cls, box = torch.randn(L, 2, pad, 10, generator=gen), torch.randn(L, 2, pad, 10, generator=gen)
    md["output_known_lbs_bboxes"] = (cls, box)
    labels, boxes, c, b, num = head.prepare_for_dn_loss(md)
    assert num == 3 * 8 and tuple(c.shape) == (L, 24, 10) and tuple(b.shape) == (L, 24, 10)
    assert labels is md["known_lbs_bboxes"][0] and boxes is md["known_lbs_bboxes"][1]
    # copy n of group k of sample s sits at query k*single + n of that sample (racformer_head.py:249-262)
    counts, single, row = (5, 3), 5, 0
    for k in range(3):
        for s, n_s in enumerate(counts):
            for n in range(n_s):
                assert torch.equal(c[:, row], cls[:, s, k * single + n]) and torch.equal(b[:, row], box[:, s, k * single + n])
                row += 1


def test_loss_says_what_is_not_built(golden_dir):
    head = small_head(np.load(os.path.join(golden_dir, "dn_input_small.npz")))
    with pytest.raises(NotImplementedError, match="racformer_amd: assigner and losses are not built"):
        head.loss(None, None, {})


# ----------------------------------------------------------------------------------- the head's forward on the tiny rig
def rig_head(query_denoising=True):
    torch.manual_seed(0)
    head = RaCFormer_head(num_classes=CFG.num_classes, in_channels=CFG.embed_dims, num_query=CFG.num_query, num_clusters=CFG.num_clusters,
                          code_size=CFG.code_size, query_denoising=query_denoising, query_denoising_groups=3,
                          transformer=dict(type="RaCFormerTransformer", **CFG.transformer_kwargs()),
                          bbox_coder=dict(type="NMSFreeCoder", post_center_range=POST_RANGE, pc_range=list(CFG.pc_range),
                                          max_num=CFG.num_query, score_threshold=0.05, num_classes=CFG.num_classes))
    syn.fill_params(head.transformer, 12)
    return head


def rig_inputs(with_gt=True):
    _, _, feats, lss, radar, metas = DG.inputs(grouped=False)
    DG.CALLS.clear()
    if with_gt:
        g = torch.Generator().manual_seed(21)
        box = torch.cat([torch.rand(2, 2, generator=g) * 60 - 30, torch.rand(2, 1, generator=g) - 1, torch.rand(2, 3, generator=g) * 3 + 0.5,
                         torch.rand(2, 3, generator=g) - 0.5], dim=1)
        metas[0]["gt_bboxes_3d"], metas[0]["gt_labels_3d"] = box, torch.tensor([1, 4])
    return feats, lss, radar, metas


@pytest.fixture
def masked_fakes(fakes, monkeypatch):  # noqa: F811
    monkeypatch.setattr(T, "sasa_fused", MR.fake_fused)
    monkeypatch.setattr(T, "sasa_backward", MR.fake_backward)
    MR.CALLS.clear()


def test_head_forward_in_training_mode(masked_fakes):
    """fails on the parent commit, whose forward raises NotImplementedError in training mode"""
    head = rig_head().train()
    feats, lss, radar, metas = rig_inputs()
    torch.manual_seed(5)
    out = head(list(feats), lss, radar, metas)
    Q, L, pad = CFG.num_query, CFG.num_layers, 3 * 2
    md = out["dn_mask_dict"]
    assert md["pad_size"] == pad and out["enc_cls_scores"] is None and out["enc_bbox_preds"] is None
    assert tuple(out["all_cls_scores"].shape) == (L, 1, Q, CFG.num_classes) and tuple(out["all_bbox_preds"].shape) == (L, 1, Q, 10)
    kc, kb = md["output_known_lbs_bboxes"]
    assert tuple(kc.shape) == (L, 1, pad, CFG.num_classes) and tuple(kb.shape) == (L, 1, pad, 10)
    # every layer's self-attention ran fused under ONE packed mask (packed once by the decoder): 6 forwards, no unfused route
    fwd = [c for c in MR.CALLS if c[0] == "fwd"]
    assert len(fwd) == L and all(c[1] for c in fwd) and fwd[0][2] is not None and len({c[2] for c in fwd}) == 1
    (out["all_cls_scores"].sum() + out["all_bbox_preds"].sum() + kc.sum() + kb.sum()).backward()
    assert len([c for c in MR.CALLS if c[0] == "bwd"]) == L and {c[2] for c in MR.CALLS} == {fwd[0][2]}
    g = head.label_enc.weight.grad
    assert g is not None and bool(torch.isfinite(g).all())
    rows = set(g.abs().sum(1).nonzero().flatten().tolist())
    assert CFG.num_classes in rows and len(rows) >= 2, "the matching queries' row and the noised labels' rows"
    assert head.init_query_bbox.weight.grad is not None
    labels, boxes, c, b, num = head.prepare_for_dn_loss(md)
    assert num == pad and tuple(c.shape) == (L, pad, CFG.num_classes)


def test_training_without_denoising_and_eval_run_unmasked(masked_fakes):
    """query_denoising=False in training mode and eval mode under grad: attn_mask None, the same launches, the same numbers"""
    feats, lss, radar, metas = rig_inputs(with_gt=False)
    head = rig_head(query_denoising=False).train()
    a = head([f.clone() for f in feats], lss, radar, metas)
    assert "dn_mask_dict" not in a and all(c[2] is None for c in MR.CALLS) and len(MR.CALLS) == CFG.num_layers
    MR.CALLS.clear()
    b = head.eval()([f.clone() for f in feats], lss, radar, rig_inputs(with_gt=False)[3])
    assert "dn_mask_dict" not in b and all(c[2] is None for c in MR.CALLS) and len(MR.CALLS) == CFG.num_layers
    assert torch.equal(a["all_cls_scores"], b["all_cls_scores"]) and torch.equal(a["all_bbox_preds"], b["all_bbox_preds"])
    assert tuple(b["all_cls_scores"].shape) == (CFG.num_layers, 1, CFG.num_query, CFG.num_classes)


def test_training_mode_without_ground_truth_says_so(masked_fakes):
    head = rig_head().train()
    feats, lss, radar, metas = rig_inputs(with_gt=False)
    with pytest.raises(NotImplementedError, match="gt_bboxes_3d"):
        head(list(feats), lss, radar, metas)
