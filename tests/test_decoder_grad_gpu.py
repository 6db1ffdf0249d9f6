"""The decoder under autograd on the MI355X: RaCFormerTransformer and RaCFormer_head (eval mode, grad enabled) are differentiable
end to end through the training route of the layer (RaCFormerTransformerDecoderLayer.forward_train), from the stacked outputs back
to every parameter, the queries, layer 0's boxes, both BEV map stacks and the un-regrouped image pyramid.

Rig: syn.SMALL6 (30 queries, 6 cameras, 2 frames), B = 1, seeded fill_params, .eval().

Gradients of one layer against the REFERENCE's own decoder layer under autograd: tests/golden/decoder_grad_small.npz
(gen_golden_decoder_grad.py; the rig and the bound in tests/decoder_grad_ref.py; CPU twin: tests/test_decoder_grad_golden_cpu.py)."""
import numpy as np
import pytest
import torch

import decoder_grad_ref as DR
from oracle import restate as R
from parity import teacher_forced_layer_check
from racformer_amd import synthetic as syn
from racformer_amd.head import RaCFormer_head
from racformer_amd.transformer import RaCFormerTransformer, regroup_pyramid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG, SEED, WSEED = syn.SMALL6, 11, 12

# Parameters that legitimately receive no gradient in the reference (at most five).
NO_GRAD_IN_REFERENCE = ()


def transformer():
    tr = RaCFormerTransformer(**CFG.transformer_kwargs()).eval()
    syn.fill_params(tr, WSEED)
    return tr.to(DEV)


def leaves():
    qb, qf = syn.make_queries(CFG, SEED)
    feats = [f.to(DEV).requires_grad_() for f in syn.make_pyramid(CFG, SEED)]
    return (qb.to(DEV).requires_grad_(), qf.to(DEV).requires_grad_(), feats, syn.make_bev(CFG, SEED, 0).to(DEV).requires_grad_(),
            syn.make_bev(CFG, SEED, 1).to(DEV).requires_grad_())


def seeded_gouts(cls, box):
    g = torch.Generator().manual_seed(3)
    return torch.randn(cls.shape, generator=g).to(DEV), torch.randn(box.shape, generator=g).to(DEV)


def run_transformer(tr):
    tr.zero_grad(set_to_none=True)
    qb, qf, feats, lss, radar = leaves()
    cls, box = tr(qb, qf, list(feats), lss, radar, None, syn.make_img_metas(CFG))
    assert cls.grad_fn is not None and box.grad_fn is not None, "the decoder's outputs carry no autograd history"
    g1, g2 = seeded_gouts(cls, box)
    ((cls * g1).sum() + (box * g2).sum()).backward()
    torch.cuda.synchronize()
    grads = {"param." + n: p.grad for n, p in tr.named_parameters()}
    grads.update(query_bbox=qb.grad, query_feat=qf.grad, lss=lss.grad, radar=radar.grad, **{f"level{l}": f.grad for l, f in enumerate(feats)})
    shapes = {"param." + n: p.shape for n, p in tr.named_parameters()}
    shapes.update(query_bbox=qb.shape, query_feat=qf.shape, lss=lss.shape, radar=radar.shape, **{f"level{l}": f.shape for l, f in enumerate(feats)})
    return cls.detach(), box.detach(), grads, shapes


@pytest.fixture(scope="module")
def first_run():
    tr = transformer()
    return tr, run_transformer(tr)


def test_transformer_is_differentiable_end_to_end(first_run):
    """THE test that fails without the training route: the fused plan's outputs have grad_fn None"""
    _, (cls, box, grads, shapes) = first_run
    assert len(NO_GRAD_IN_REFERENCE) <= 5
    for name, g in grads.items():
        if name.startswith("param.") and name[len("param."):] in NO_GRAD_IN_REFERENCE:
            continue
        assert g is not None, f"{name}: no gradient"
        assert g.shape == shapes[name], name           # (pyramid levels: the original [B,T*N,G*C,H,W])
        assert bool(torch.isfinite(g).all()), f"{name}: non-finite gradient"
        assert bool((g != 0).any()), f"{name}: gradient identically zero"
    assert bool((grads["query_bbox"][..., 8:] == 0).all()), "the reference detaches the velocity"
    assert bool((grads["query_bbox"][..., :8] != 0).any(dim=1).all()), "every other box component takes part"


def test_training_route_is_deterministic_where_nothing_scatters(first_run):
    """two runs: bitwise equal, except what atomic scatters feed (the pyramid levels, the BEV value streams and what lies upstream
    of them: the map stacks, value_proj, the positional embeddings, the radar stream's temporal encoder) -- 1e-5 of the largest
    element there"""
    tr, _ = first_run
    # (first_run was the process's first pass through the library GEMMs and convolutions, whose first call selects an algorithm:
    #  the two runs compared here both come after it)
    cls, box, grads, _ = run_transformer(tr)
    cls2, box2, grads2, _ = run_transformer(tr)
    print("\nforward, two runs: max |diff| cls %.3e box %.3e" % (float((cls - cls2).abs().max()), float((box - box2).abs().max())))
    for name, g in grads.items():
        d = float((g - grads2[name]).abs().max())
        if d:
            print(f"  {name}: max |diff| {d:.3e} of max {float(g.abs().max()):.3e}")
    assert torch.equal(cls, cls2) and torch.equal(box, box2)
    scattered = ("level", "lss", "radar", "param.decoder.decoder_layer.sampling_radar_bev.temporal_encoder.",
                 "param.decoder.decoder_layer.sampling_radar_bev.attention.value_proj.", "param.decoder.decoder_layer.sampling_lss_bev.attention.value_proj.",
                 "param.decoder.decoder_layer.sampling_radar_bev.positional_encoding.", "param.decoder.decoder_layer.sampling_lss_bev.positional_encoding.")
    for name, g in grads.items():
        if name.startswith(scattered):
            assert float((g - grads2[name]).abs().max()) <= 1e-5 * float(g.abs().max()), name
        else:
            assert torch.equal(g, grads2[name]), f"{name}: two runs differ"


def test_head_in_eval_mode_reaches_its_embeddings():
    torch.manual_seed(0)                               # (the embedding's free columns are drawn N(0,1) by the constructor)
    head = RaCFormer_head(num_classes=CFG.num_classes, in_channels=CFG.embed_dims, num_query=CFG.num_query, num_clusters=CFG.num_clusters,
                          code_size=CFG.code_size, transformer=dict(type="RaCFormerTransformer", **CFG.transformer_kwargs()),
                          bbox_coder=dict(type="NMSFreeCoder", post_center_range=[-61.2, -61.2, -10.0, 61.2, 61.2, 10.0],
                                          pc_range=list(CFG.pc_range), max_num=CFG.num_query, score_threshold=0.05,
                                          num_classes=CFG.num_classes)).eval()
    syn.fill_params(head.transformer, WSEED)
    head = head.to(DEV)
    _, _, feats, lss, radar = leaves()
    out = head(list(feats), lss, radar, syn.make_img_metas(CFG))
    cls, box = out["all_cls_scores"], out["all_bbox_preds"]
    assert cls.grad_fn is not None and box.grad_fn is not None
    g1, g2 = seeded_gouts(cls, box)
    ((cls * g1).sum() + (box * g2).sum()).backward()
    for emb in (head.init_query_bbox, head.label_enc):
        g = emb.weight.grad
        assert g is not None and bool(torch.isfinite(g).all()) and bool((g != 0).any())
    assert all(f.grad is not None and bool((f.grad != 0).any()) for f in feats)
    head.train()
    with pytest.raises(NotImplementedError):
        head(list(feats), lss, radar, syn.make_img_metas(CFG))


def test_training_route_computes_the_layer():
    """one layer, the same inputs under grad (forward_train: exact fp32 torch GEMMs) and under no_grad (forward_fused: split
    precision): the teacher-forced per-layer criterion of tests/parity.py, 1e-4 on every query and every stage, class argmax
    identical up to fp32 ties.  (Not bitwise: the routes differ in arithmetic.)"""
    tr = transformer()
    dec, layer = tr.decoder, tr.decoder.decoder_layer
    metas = syn.make_img_metas(CFG)
    dec.stage_metas(metas, 1, torch.device(DEV))
    qb, qf = (t.to(DEV) for t in syn.make_queries(CFG, SEED))
    lss, radar = syn.make_bev(CFG, SEED, 0).to(DEV), syn.make_bev(CFG, SEED, 1).to(DEV)
    with torch.no_grad():
        feats = regroup_pyramid([f.to(DEV) for f in syn.make_pyramid(CFG, SEED)], CFG.num_cams)

    def run(layer_index):
        st = {}
        layer._carry, layer.sampling.capture_loc = None, []
        feat, cls, box = layer(qb, qf, feats, lss, radar, None, metas, layer=layer_index, stages=st)
        torch.cuda.synchronize()
        views = R.views_of(layer.sampling.capture_loc[0].cpu(), CFG.num_cams)
        layer.sampling.capture_loc = None
        return feat, cls, box, {k: v.detach().cpu() for k, v in st.items()}, views

    for l in (0, CFG.num_layers - 1):                 # (the widest and the narrowest d_region)
        with torch.no_grad():
            rfeat, rcls, rbox, rst, rviews = run(l)
        assert rfeat.grad_fn is None
        feat, cls, box, st, views = run(l)
        assert feat.grad_fn is not None and cls.grad_fn is not None and box.grad_fn is not None
        Q = CFG.num_query
        g = dict(in_feat=np.zeros((1, 1)), out_feat_last=rfeat.cpu().numpy(), out_cls=[None] * l + [rcls.cpu().numpy()],
                 out_box=[None] * l + [rbox.cpu().numpy()], views=[None] * l + [np.asarray(rviews)], probe_q=np.arange(Q),
                 probe_q_sampling=np.arange(Q), **{"stage_" + k: [None] * l + [v.numpy()] for k, v in rst.items()})
        # (in_feat has one "layer", so the check reads out_feat_last as this layer's reference features)
        g["in_feat"] = np.zeros((l + 1, 1))
        flips = teacher_forced_layer_check(l, g, CFG, feat.detach().cpu(), cls.detach().cpu(), box.detach().cpu(), st, views, what="training route")
        assert flips == 0, "the two routes run the same sampling kernel on the same inputs"
        a, b = cls.detach().argmax(-1), rcls.argmax(-1)
        top2 = rcls.topk(2, dim=-1).values
        tie = (top2[..., 0] - top2[..., 1]).abs() <= 2e-4 * top2[..., 0].abs()
        assert bool(((a == b) | tie).all()), "class argmax differs away from an fp32 tie"


def test_layer_gradients_against_the_reference(golden_dir):
    """one layer of the training route on the fixture's inputs and weights: per gradient tensor, the error against the reference's
    float64 gradient over the tensor's largest element <= max(2 x the reference's own float32 figure, 1e-5); the outputs within
    1e-5 of their largest element"""
    g = DR.load_golden(golden_dir)
    layer = DR.build_layer(g, device=DEV)
    out, grads = DR.run_layer(layer, g, device=DEV)
    report = []
    bad = DR.check_against_golden(g, out, grads, "training route", report)
    worst = sorted(report, key=lambda r: -r[1] / r[3])[:8]
    print("\nclosest to the bound:", ", ".join(f"{k} {e:.1e} (ref {r:.1e})" for k, e, r, _ in worst))
    assert not bad, "\n".join(bad)
