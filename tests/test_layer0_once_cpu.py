"""Layer 0's query-only front half, once per weights (RaCFormerTransformerDecoderLayer.layer0_block): the host logic that
decides whether a call may take the route and what a stored block is valid for -- no GPU.  The fused plan itself is replaced
by a recorder (it needs the GPU); what reaches it as ``query_key`` is under test."""
import ctypes

import pytest
import torch

from racformer_amd import _lib
from racformer_amd import synthetic as syn
from racformer_amd import transformer as T

CFG = syn.SMALL
KEY = ("init_queries", 1234, 0, 5678, 0, "cpu", 1)


@pytest.fixture(scope="module")
def transformer():
    tr = T.RaCFormerTransformer(**CFG.transformer_kwargs()).eval()
    syn.fill_params(tr, 12)
    for p in tr.parameters():
        p.requires_grad_(False)
    return tr


@pytest.fixture
def seen(monkeypatch):
    """forward_fused / forward_train replaced by recorders of the key they were given; the fused plan's CUDA gate lifted"""
    calls = []

    def fused(self, query_bbox, query_feat, mlvl_feats, img_metas, layer, prepared, stages=None, out_slots=None, query_key=None):
        calls.append(("forward_fused", layer, query_key))
        self.last_bbox_xy = query_bbox
        return query_feat, query_feat[..., :10], query_bbox

    def train(self, query_bbox, query_feat, mlvl_feats, attn_mask, img_metas, layer, prepared, stages=None):
        calls.append(("forward_train", layer, None))
        self.last_bbox_xy = query_bbox
        return query_feat, query_feat[..., :10], query_bbox
    cls = T.RaCFormerTransformerDecoderLayer
    monkeypatch.setattr(cls, "forward_fused", fused)
    monkeypatch.setattr(cls, "forward_train", train)
    monkeypatch.setattr(cls, "fused_plan_applies", lambda self, query_feat, attn_mask: attn_mask is None)
    monkeypatch.setattr(cls, "prepare", lambda self, lss, radar: {})
    monkeypatch.setattr(cls, "prepare_train", lambda self, lss, radar: {"train": True})
    return calls


def call_layer(module, **kw):
    qb, qf = syn.make_queries(CFG, 3)
    lss = torch.zeros(1, CFG.num_frames, CFG.embed_dims, 2, 2)
    return module(qb, qf, [], lss, lss, kw.pop("attn_mask", None), syn.make_img_metas(CFG), **kw)


def test_a_key_reaches_layer_0_only(transformer, seen, monkeypatch):
    dec = transformer.decoder
    monkeypatch.setattr(dec, "stage_metas", lambda *a: None)
    monkeypatch.setattr(T, "regroup_pyramid", lambda feats, *a: feats)
    qb, qf = syn.make_queries(CFG, 3)
    lss = torch.zeros(1, CFG.num_frames, CFG.embed_dims, 2, 2)
    with torch.no_grad():
        transformer(qb, qf, [], lss, lss, None, syn.make_img_metas(CFG), raw=True, query_key=KEY)
    assert seen == [("forward_fused", 0, KEY)] + [("forward_fused", i, None) for i in range(1, CFG.num_layers)]


def test_a_missing_key_takes_todays_path(transformer, seen):
    layer = transformer.decoder.decoder_layer
    with torch.no_grad():
        call_layer(layer)
        call_layer(layer, layer=0, query_key=None)
    assert seen == [("forward_fused", 0, None)] * 2
    assert layer._layer0_block is None


def test_autograd_on_takes_todays_path(transformer, seen):
    layer = transformer.decoder.decoder_layer
    call_layer(layer, query_key=KEY)                    # grad mode, everything frozen: the fused plan, without the route
    layer.norm3.bias.requires_grad_(True)
    try:
        call_layer(layer, query_key=KEY)                # something requires grad: the training route
    finally:
        layer.norm3.bias.requires_grad_(False)
    with torch.no_grad():
        call_layer(layer, query_key=KEY)
    assert seen == [("forward_fused", 0, None), ("forward_train", 0, None), ("forward_fused", 0, KEY)]


def test_an_attention_mask_takes_todays_path(transformer, seen):
    layer = transformer.decoder.decoder_layer
    mask = torch.zeros(CFG.num_query, CFG.num_query, dtype=torch.bool)
    with torch.no_grad():
        call_layer(layer, query_key=KEY, attn_mask=mask)
    assert seen == [("forward_train", 0, None)]
    assert not layer.layer0_once_applies(KEY, 0, mask)


def test_the_gate(transformer):
    layer = transformer.decoder.decoder_layer
    with torch.no_grad():
        assert layer.layer0_once_applies(KEY, 0, None)
        assert not layer.layer0_once_applies(None, 0, None)
        assert not layer.layer0_once_applies(KEY, 1, None)
        for switch in ("layer0_once", "rowgemm", "fused"):
            setattr(layer, switch, False)
            try:
                assert not layer.layer0_once_applies(KEY, 0, None), switch
            finally:
                setattr(layer, switch, True)
    assert not layer.layer0_once_applies(KEY, 0, None)          # autograd on


def prepared_for(layer):
    w, b, widths = layer._wide_linears()
    return dict(wide_w=w, wide_b=b, wide_widths=widths, wide_img=(None, None), split_packs={}, sasa_w=layer.self_attn.wide_in_proj())


def test_signature_is_a_pure_function(transformer):
    """same arguments, same weights -> equal signatures; an in-place update, a replaced parameter, load_state_dict, another key,
    pc_range, plan switch or shape -> another one"""
    layer = transformer.decoder.decoder_layer
    qb, qf = syn.make_queries(CFG, 3)
    with torch.no_grad():
        prep = prepared_for(layer)
        sig = layer.layer0_signature(KEY, qb, qf, prep)
        assert sig == layer.layer0_signature(KEY, qb, qf, prep)
        assert hash(sig) == hash(layer.layer0_signature(KEY, qb, qf, dict(prep)))
        assert layer._layer0_block is None                                   # (computing it stores nothing)
        assert sig != layer.layer0_signature(KEY[:-1] + (2,), qb, qf, prep)
        assert sig != layer.layer0_signature(KEY, qb.clone(), qf, prep)
        assert sig != layer.layer0_signature(KEY, qb, qf[:, :-1], prep)
        feeders = [layer.position_encoder[0].bias, layer.position_encoder[4].weight, layer.self_attn.attention.attn.in_proj_weight,
                   layer.self_attn.gen_tau.bias, layer.self_attn.attention.attn.out_proj.bias, layer.norm1.weight,
                   layer.sampling.scale_weights.bias, layer.sampling_lss_bev.attention.bev_queue_weight.weight,
                   layer.mixing.parameter_generator.weight, layer.mixing.parameter_generator.bias]
        for p in feeders:
            before = layer.layer0_signature(KEY, qb, qf, prep)
            p.mul_(1.0)                                                     # same values, another version
            assert before != layer.layer0_signature(KEY, qb, qf, prep)
        # what the chain does not read leaves it alone
        before = layer.layer0_signature(KEY, qb, qf, prep)
        layer.norm3.weight.mul_(1.0)
        layer.ffn.layers[1].bias.mul_(1.0)
        assert before == layer.layer0_signature(KEY, qb, qf, prep)
        layer.load_state_dict(layer.state_dict())
        assert before != layer.layer0_signature(KEY, qb, qf, prep)
        before = layer.layer0_signature(KEY, qb, qf, prep)
        layer.split_gemm = False
        try:
            assert before != layer.layer0_signature(KEY, qb, qf, prep)
        finally:
            layer.split_gemm = True
        pc = layer.pc_range
        layer.pc_range = [v * 2 for v in pc]
        try:
            assert before != layer.layer0_signature(KEY, qb, qf, prep)
        finally:
            layer.pc_range = pc
        assert before == layer.layer0_signature(KEY, qb, qf, prep)


def test_mixing_row_period_arguments():
    """a period that does not divide the rows is refused before any launch (argument validation needs no GPU)"""
    lib = _lib.lib()
    p8 = ctypes.c_void_p(8)
    width = 4 * (64 * 64 + 128 * 24)
    for period in (0, 4, 7):
        rc = lib.rac_mixing_period_fwd(p8, p8, 1.0, p8, None, 1.0, width, period, 6, 4, 24, 64, 128, 1e-5, 0, None)
        assert rc == -1 and b"period" in lib.rac_last_error(), period
