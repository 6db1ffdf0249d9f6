"""RaCFormer_head in training mode on the MI355X, on the tiny rig of tests/test_decoder_grad_gpu.py (syn.SMALL6, B = 1): the
denoising queries in front of the matching queries, the decoder under their mask through the masked SASA kernels, the outputs
split at pad_size; a backward from the sum of all outputs reaches every parameter the eval-mode backward reaches, plus the noised
labels' rows of label_enc; and the mask isolates the matching queries from the denoising part bit for bit."""
import pytest
import torch

from racformer_amd import synthetic as syn
from racformer_amd.head import RaCFormer_head
from test_decoder_grad_gpu import CFG, DEV, WSEED, leaves

pytestmark = pytest.mark.gpu
GROUPS = 3


def make_head():
    torch.manual_seed(0)                               # (the embedding's free columns are drawn N(0,1) by the constructor)
    head = RaCFormer_head(num_classes=CFG.num_classes, in_channels=CFG.embed_dims, num_query=CFG.num_query, num_clusters=CFG.num_clusters,
                          code_size=CFG.code_size, query_denoising=True, query_denoising_groups=GROUPS,
                          transformer=dict(type="RaCFormerTransformer", **CFG.transformer_kwargs()),
                          bbox_coder=dict(type="NMSFreeCoder", post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                                          pc_range=list(CFG.pc_range), max_num=CFG.num_query, score_threshold=0.05,
                                          num_classes=CFG.num_classes))
    syn.fill_params(head.transformer, WSEED)
    return head.to(DEV)


def metas_with_gt(n=3):
    metas = syn.make_img_metas(CFG)
    g = torch.Generator().manual_seed(21)
    box = torch.cat([torch.rand(n, 2, generator=g) * 60 - 30, torch.rand(n, 1, generator=g) - 1, torch.rand(n, 3, generator=g) * 3 + 0.5,
                     torch.rand(n, 3, generator=g) - 0.5], dim=1)
    metas[0]["gt_bboxes_3d"], metas[0]["gt_labels_3d"] = box, torch.arange(n) % CFG.num_classes     # (CPU tensors: moved with .to)
    return metas


def run(head, seed, backward=False):
    head.zero_grad(set_to_none=True)
    _, _, feats, lss, radar = leaves()
    torch.manual_seed(seed)                            # the noise of the denoising part
    out = head(list(feats), lss, radar, metas_with_gt())
    if backward:
        md = out["dn_mask_dict"]
        total = out["all_cls_scores"].sum() + out["all_bbox_preds"].sum() + sum(x.sum() for x in md["output_known_lbs_bboxes"])
        total.backward()
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def head():
    return make_head()


def test_training_forward_and_backward(head):
    """fails on the parent commit, whose forward raises in training mode"""
    out = run(head.train(), seed=1, backward=True)
    L, Q, pad = CFG.num_layers, CFG.num_query, GROUPS * 3
    md = out["dn_mask_dict"]
    assert md["pad_size"] == pad == GROUPS * 3                              # dn_single_pad * dn_group_num (:205-206)
    assert tuple(out["all_cls_scores"].shape) == (L, 1, Q, CFG.num_classes) and tuple(out["all_bbox_preds"].shape) == (L, 1, Q, 10)
    kc, kb = md["output_known_lbs_bboxes"]
    assert tuple(kc.shape) == (L, 1, pad, CFG.num_classes) and tuple(kb.shape) == (L, 1, pad, 10)
    assert md["map_known_indice"].numel() == md["known_indice"].numel() == pad and md["known_indice"].is_cuda
    for x in (out["all_cls_scores"], out["all_bbox_preds"], kc, kb):
        assert x.grad_fn is not None and bool(torch.isfinite(x).all())
    train_grads = {n: p.grad for n, p in head.named_parameters()}
    noised = head.label_enc.weight.grad.abs().sum(1).nonzero().flatten().tolist()
    # the same backward in eval mode (grad enabled): every parameter that gets a gradient there gets a finite one in training
    head.eval()
    head.zero_grad(set_to_none=True)
    _, _, feats, lss, radar = leaves()
    ev = head(list(feats), lss, radar, syn.make_img_metas(CFG))
    assert "dn_mask_dict" not in ev
    (ev["all_cls_scores"].sum() + ev["all_bbox_preds"].sum()).backward()
    n_eval = 0
    for n, p in head.named_parameters():
        if p.grad is not None:
            n_eval += 1
            assert train_grads[n] is not None and bool(torch.isfinite(train_grads[n]).all()), n
    assert n_eval > 50
    eval_rows = head.label_enc.weight.grad.abs().sum(1).nonzero().flatten().tolist()
    assert eval_rows == [CFG.num_classes] and CFG.num_classes in noised and len(noised) > 1, "label_enc rows of the noised labels"


def test_mask_isolates_the_matching_queries_bitwise(head):
    """two runs whose denoising parts carry different noise: the matching queries' outputs are the same bits (a blocked pair
    contributes an exact zero, a row's order of summation does not depend on other rows), the denoising outputs differ"""
    head.train()
    with torch.no_grad():
        a, b = run(head, seed=1), run(head, seed=2)
    ka, kb = a["dn_mask_dict"]["output_known_lbs_bboxes"], b["dn_mask_dict"]["output_known_lbs_bboxes"]
    assert not torch.equal(ka[0], kb[0]) and not torch.equal(ka[1], kb[1]), "the two runs must differ in their noise"
    assert torch.equal(a["all_cls_scores"], b["all_cls_scores"])
    assert torch.equal(a["all_bbox_preds"], b["all_bbox_preds"])
