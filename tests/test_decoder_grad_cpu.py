"""Routing of the decoder layer by autograd state, without a GPU: which plan a call takes, what regroup_pyramid launches, and what
prepare() hands out under the gate of the training route.  The HIP launchers are replaced by fakes that behave like the real ones
(plain tensors in and out, no autograd history), following tests/test_racsampling_grad_cpu.py; the last test runs one whole layer
through forward_train on those fakes and checks that a gradient reaches every parameter and input."""
import ctypes
import os
import re

import pytest
import torch

import bev_sampling_ref as BR
import refine_ref as RR
import sampling4d_core_ref as SR
import test_sasa_grad_cpu as SA
from racformer_amd import _lib
from racformer_amd import synthetic as syn
from racformer_amd import transformer as T

CFG = syn.SMALL6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = []


def fake_regroup(feats, dims, groups, out_dtype=torch.float32):
    CALLS.append(("regroup_fwd", len(feats), dims, groups, out_dtype, any(f.requires_grad for f in feats) and torch.is_grad_enabled()))
    B, Tn, N, C = dims
    with torch.no_grad():
        return [f.view(B, Tn, N, groups, C, *f.shape[3:]).permute(0, 1, 3, 2, 5, 6, 4).reshape(B * Tn * groups, N, *f.shape[3:], C)
                .contiguous().to(out_dtype) for f in feats]


def fake_regroup_backward(grads, dims, groups):
    CALLS.append(("regroup_bwd", len(grads)))
    B, Tn, N, C = dims
    for g in grads:
        if g.dtype != torch.float32:
            raise RuntimeError("regroup_backward: float32 features only")
    return [g.view(B, Tn, groups, N, *g.shape[2:4], C).permute(0, 1, 3, 2, 6, 4, 5).reshape(B, Tn * N, groups * C, *g.shape[2:4]).contiguous()
            for g in grads]


def fake_refine(proposal, delta, time_diff_safe, num_ray):
    CALLS.append(("refine_fwd",))
    with torch.no_grad():
        return RR.forward(proposal, delta, time_diff_safe, num_ray)


def fake_refine_backward(proposal, delta, time_diff_safe, num_ray, grad_pred=None, grad_xy=None):
    CALLS.append(("refine_bwd", grad_pred is not None, grad_xy is not None))
    gd, gp = RR.closed_form_bwd(proposal, delta, time_diff_safe, num_ray, grad_pred, grad_xy)
    return gd.to(delta.dtype), gp.to(proposal.dtype)


@pytest.fixture
def fakes(monkeypatch):
    monkeypatch.setattr(T, "regroup_fused", fake_regroup)
    monkeypatch.setattr(T, "regroup_backward", fake_regroup_backward)
    monkeypatch.setattr(T, "refine_fused", fake_refine)
    monkeypatch.setattr(T, "refine_backward", fake_refine_backward)
    monkeypatch.setattr(T, "sampling4d_fused", SR.fake_fused)
    monkeypatch.setattr(T, "sampling4d_backward", SR.fake_backward)
    monkeypatch.setattr(T, "bev_sampling_fused", BR.fake_fused)
    monkeypatch.setattr(T, "bev_sampling_backward", BR.fake_backward)
    monkeypatch.setattr(T, "sasa_fused", SA.fake_fused)
    monkeypatch.setattr(T, "sasa_backward", SA.fake_backward)
    monkeypatch.setattr(T, "box_prep", lambda qb, pc: T.box_table_torch(qb.detach(), pc).detach())
    CALLS.clear()


@pytest.fixture
def routes(monkeypatch):
    """the two plans of the layer replaced by recorders (the fused plan needs the GPU; here only the choice is under test)"""
    def fused(self, query_bbox, query_feat, *a, **k):
        CALLS.append(("forward_fused",))
        return query_feat, query_feat[..., :10], query_bbox

    def train(self, query_bbox, query_feat, *a, **k):
        CALLS.append(("forward_train",))
        return query_feat, query_feat[..., :10], query_bbox
    monkeypatch.setattr(T.RaCFormerTransformerDecoderLayer, "forward_fused", fused)
    monkeypatch.setattr(T.RaCFormerTransformerDecoderLayer, "forward_train", train)
    # (forward_fused is gated on CUDA tensors: the recorder stands for it on this machine)
    monkeypatch.setattr(T.RaCFormerTransformerDecoderLayer, "fused_plan_applies", lambda self, query_feat, attn_mask: attn_mask is None)


@pytest.fixture(scope="module")
def transformer():
    tr = T.RaCFormerTransformer(**CFG.transformer_kwargs()).eval()
    syn.fill_params(tr, 12)
    return tr


def inputs(seed=11, grouped=True):
    qb, qf = syn.make_queries(CFG, seed)
    feats = syn.make_pyramid(CFG, seed)
    if grouped:
        feats = fake_regroup(feats, (1, CFG.num_frames, CFG.num_cams, CFG.channels), 4)
        CALLS.clear()
    metas = syn.make_img_metas(CFG)
    return qb, qf, feats, syn.make_bev(CFG, seed, 0), syn.make_bev(CFG, seed, 1), metas


def set_requires_grad(module, flag):
    for p in module.parameters():
        p.requires_grad_(flag)


def cache_tensors(obj):
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from cache_tensors(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from cache_tensors(v)


def test_inference_calls_take_forward_fused(transformer, routes, monkeypatch):
    layer = transformer.decoder.decoder_layer
    monkeypatch.setattr(layer, "prepare", lambda lss, radar: CALLS.append(("prepare", False)) or {})    # (today's signature)
    monkeypatch.setattr(layer, "prepare_train", lambda lss, radar: CALLS.append(("prepare", True)) or {"train": True})
    qb, qf, feats, lss, radar, metas = inputs()
    set_requires_grad(layer, True)
    with torch.no_grad():
        layer(qb, qf, feats, lss, radar, None, metas)
    with torch.inference_mode():
        layer(qb, qf, feats, lss, radar, None, metas)
    set_requires_grad(layer, False)
    layer(qb, qf, feats, lss, radar, None, metas)                # grad mode, everything frozen
    assert [c for c in CALLS if c[0] != "prepare"] == [("forward_fused",)] * 3
    assert [c for c in CALLS if c[0] == "prepare"] == [("prepare", False)] * 3


@pytest.mark.parametrize("what", ["parameter", "query_feat", "query_bbox", "pyramid level", "lss", "radar"])
def test_anything_requiring_grad_takes_the_training_route(transformer, routes, monkeypatch, what):
    layer = transformer.decoder.decoder_layer
    monkeypatch.setattr(layer, "prepare", lambda lss, radar: CALLS.append(("prepare", False)) or {})    # (today's signature)
    monkeypatch.setattr(layer, "prepare_train", lambda lss, radar: CALLS.append(("prepare", True)) or {"train": True})
    qb, qf, feats, lss, radar, metas = inputs()
    set_requires_grad(layer, False)
    try:
        if what == "parameter":
            layer.norm3.bias.requires_grad_(True)
        else:
            {"query_feat": qf, "query_bbox": qb, "pyramid level": feats[2], "lss": lss, "radar": radar}[what].requires_grad_(True)
        layer(qb, qf, feats, lss, radar, None, metas)
        # (a prepared dict built for inference is not used under the gate)
        layer(qb, qf, feats, lss, radar, None, metas, prepared={"wide_w": None})
        with torch.no_grad():
            layer(qb, qf, feats, lss, radar, None, metas)
    finally:
        set_requires_grad(layer, True)
    assert CALLS == [("prepare", True), ("forward_train",), ("prepare", True), ("forward_train",), ("prepare", False), ("forward_fused",)]


def test_regroup_pyramid_launches_what_it_launched_before(fakes):
    feats = syn.make_pyramid(CFG, 3)
    dims = (1, CFG.num_frames, CFG.num_cams, CFG.channels)
    with torch.no_grad():
        a = T.regroup_pyramid(list(feats), CFG.num_cams, 4)
    with torch.inference_mode():
        T.regroup_pyramid(list(feats), CFG.num_cams, 4)
    T.regroup_pyramid(list(feats), CFG.num_cams, 4, out_dtype=torch.bfloat16)       # grad mode, nothing requires grad
    assert CALLS == [("regroup_fwd", 4, dims, 4, torch.float32, False)] * 2 + [("regroup_fwd", 4, dims, 4, torch.bfloat16, False)]
    assert all(o.grad_fn is None for o in a)
    CALLS.clear()
    feats[1].requires_grad_()
    feats[3].requires_grad_()
    outs = T.regroup_pyramid(list(feats), CFG.num_cams, 4)
    assert all(torch.equal(o, p) for o, p in zip(outs, a)) and all(o.grad_fn is not None for o in outs)
    gouts = [torch.randn_like(o) for o in outs]
    torch.autograd.backward(outs, gouts)
    assert CALLS == [("regroup_fwd", 4, dims, 4, torch.float32, False), ("regroup_bwd", 2)]    # (no history inside the launcher)
    assert feats[0].grad is None and feats[2].grad is None
    for l in (1, 3):
        h, w = feats[l].shape[3:]
        want = gouts[l].view(1, CFG.num_frames, 4, CFG.num_cams, h, w, CFG.channels).permute(0, 1, 3, 2, 6, 4, 5).reshape(feats[l].shape)
        assert torch.equal(feats[l].grad, want)


def test_regroup_bf16_raises_at_backward_time(fakes):
    feats = [f.requires_grad_() for f in syn.make_pyramid(CFG, 3)[:2]]
    outs = T.regroup_pyramid(feats, CFG.num_cams, 4, out_dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="float32 features only"):
        torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])


def test_prepare_serves_the_cache_to_inference_and_live_operands_to_training(transformer):
    layer = transformer.decoder.decoder_layer
    layer._pack_cache.clear()
    _, _, _, lss, radar, _ = inputs()
    set_requires_grad(layer, True)
    with torch.no_grad():
        a = layer.prepare(lss, radar)
        b = layer.prepare(lss, radar)
    assert not a.get("train") and a["wide_w"] is b["wide_w"] and a["sasa_w"][0] is b["sasa_w"][0] and a["c0r0_w"] is b["c0r0_w"]
    assert not any(t.requires_grad for t in cache_tensors(a))
    cached = {k: v[0] for k, v in layer._pack_cache.items()}
    p = layer.prepare(lss, radar)                                                                      # under the gate
    assert p["train"] and not p["split_packs"] and p["wide_img"] == (None, None) and p["value_scales"] is None
    for key in ("wide_w", "wide_b", "out_proj_split", "lss_value", "radar_value"):
        assert p[key].requires_grad and p[key].grad_fn is not None, key
    assert all(t.requires_grad for t in p["sasa_w"])
    assert not any(k in p for k in ("bev_owt", "c0r0_w", "fusion_k", "ffn2_k")), "operands of forward_fused carry no history: not handed out"
    assert {k: v[0] for k, v in layer._pack_cache.items()} == cached, "the training route must not touch the cache"
    assert not any(t.grad_fn is not None or t.requires_grad for t in cache_tensors({k: v[1] for k, v in layer._pack_cache.items()}))
    # each of the eleven Linears receives its gradient through the one wide operand
    (p["wide_w"].sum() + p["wide_b"].sum()).backward()
    for m in (layer.sampling.sampling_offset, layer.sampling_radar_bev.attention.bev_queue_weight, layer.sampling_lss_bev.scale_weights):
        assert m.weight.grad is not None and m.bias.grad is not None
    transformer.zero_grad(set_to_none=True)
    # frozen parameters, a BEV stack that requires grad: the gate holds, the value stream carries the history
    set_requires_grad(layer, False)
    try:
        q = layer.prepare(lss.clone().requires_grad_(), radar)
        assert q["train"] and q["lss_value"].requires_grad and not q["radar_value"].requires_grad
        assert not layer.prepare(lss, radar).get("train")
        assert layer.prepare_train(lss, radar)["train"]                      # what a caller takes that knows of a query requiring grad
    finally:
        set_requires_grad(layer, True)


def test_int16_value_storage_raises_under_the_gate(transformer):
    layer = transformer.decoder.decoder_layer
    _, _, _, lss, radar, _ = inputs()
    layer.value_storage = "i16"
    try:
        with pytest.raises(RuntimeError, match="int16 block-stored value stream has no gradient path"):
            layer.prepare(lss, radar)
        with torch.no_grad():
            layer.prepare(lss, radar)                     # (a preference without a GPU: fp32 streams, as before)
    finally:
        layer.value_storage = "f32"


def test_new_symbols_are_exported_with_the_headers_signatures():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "racformer_hip.h")).read(), flags=re.S)
    want = {"rac_regroup_bwd": "pp" + "i" * 7 + "p", "rac_regroup_multi_bwd": "ippp" + "i" * 5 + "p", "rac_refine_bwd": "p" * 7 + "iii" + "fp"}
    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_float: "f"}
    lib = _lib.lib()
    for name, sig in want.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text).group(1)
        parsed = "".join("p" if "*" in x else ("f" if x.strip().startswith("float") else "i") for x in params.split(","))
        assert parsed == sig, name
        assert "".join(kind[a] for a in _lib.SIGNATURES[name][1]) == sig and hasattr(lib, name)
    # argument checks run before any HIP call
    assert lib.rac_regroup_bwd(None, None, 1, 1, 1, 1, 4, 2, 2, None) == -1 and b"null pointer" in lib.rac_last_error()
    one = (ctypes.c_void_p * 1)(8)
    hw = (ctypes.c_int32 * 2)(3, 5)
    assert lib.rac_regroup_multi_bwd(1, one, one, hw, 1, 1, 1, 1, 4, None) == -1 and b"H*W % 4" in lib.rac_last_error()
    assert lib.rac_regroup_multi_bwd(9, one, one, hw, 1, 1, 1, 1, 4, None) == -1
    assert lib.rac_refine_bwd(None, None, None, None, None, None, None, 1, 1, 1, 150.0, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_refine_bwd(None, None, None, None, None, None, None, 0, 5, 1, 150.0, None) == 0


def test_one_layer_through_the_training_route_reaches_everything(transformer, fakes):
    """forward_train on the fakes: outputs with history, a finite gradient at every parameter of the layer and every input; the
    detached bbox_pred reaches the refine backward as an absent gradient; _carry untouched, no slots written"""
    layer = transformer.decoder.decoder_layer
    set_requires_grad(layer, True)
    transformer.zero_grad(set_to_none=True)
    qb, qf, feats, lss, radar, metas = inputs()
    transformer.decoder.stage_metas(metas, 1, qb.device)
    leaves = [t.requires_grad_() for t in (qb, qf, lss, radar, *feats)]
    layer._carry = marker = ("kept",)
    layer.wrote_slots = False
    stages = {}
    x, cls, pred = layer(qb, qf, feats, lss, radar, None, metas, layer=0, stages=stages)
    xy = layer.last_bbox_xy
    assert layer._carry is marker and layer.wrote_slots is False
    assert all(t.grad_fn is not None for t in (x, cls, pred, xy))
    assert set(stages) == {"position_encoder", "self_attn", "sampling_radar_bev", "sampling_lss_bev", "sampling", "mixing", "ffn"}
    g = torch.Generator().manual_seed(1)
    (cls * torch.randn(cls.shape, generator=g)).sum().add((xy * torch.randn(xy.shape, generator=g)).sum()).backward()
    assert ("refine_bwd", False, True) in CALLS
    # (x feeds the next layer only: norm3 is reached through cls / reg; the generic head of one layer leaves nothing out)
    for name, p in layer.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    for t in leaves:
        assert t.grad is not None and bool(torch.isfinite(t.grad).all()) and bool((t.grad != 0).any())
    assert bool((qb.grad[..., 8:] == 0).all())
    transformer.zero_grad(set_to_none=True)
