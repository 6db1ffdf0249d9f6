"""Layer 0's query-only front half, once per weights (RaCFormerTransformerDecoderLayer.layer0_block), on the GPU: the route
reproduces the per-call computation bit for bit (every kernel on the chain is deterministic; the block is filled by the
launches a call without a key issues), at B = 1 and B = 2; a weight update invalidates the block; a hit launches five
self-attentions and five generator GEMMs instead of six; captured plans read one shared block; and the mixing kernels' parameter
row period (rac_mixing_period_fwd) against stacked parameters."""
from dataclasses import replace

import pytest
import torch

from racformer_amd import _lib
from racformer_amd import synthetic as syn
from racformer_amd.fused import SPLIT_ACT_SCALE, mixing_fused
from racformer_amd.graph import CapturedForward, CapturedStep
from racformer_amd.head import RaCFormer_head

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STAGES = ("position_encoder", "self_attn", "sampling_radar_bev", "sampling_lss_bev", "sampling", "mixing", "ffn")
POST_RANGE = [-61.2, -61.2, -10.0, 61.2, 61.2, 10.0]


def make_head(cfg, wseed=12):
    head = RaCFormer_head(
        num_classes=cfg.num_classes, in_channels=cfg.embed_dims, num_query=cfg.num_query, num_clusters=cfg.num_clusters,
        code_size=cfg.code_size, transformer=dict(type="RaCFormerTransformer", **cfg.transformer_kwargs()),
        bbox_coder=dict(type="NMSFreeCoder", post_center_range=POST_RANGE, pc_range=list(cfg.pc_range), max_num=30,
                        score_threshold=0.05, num_classes=cfg.num_classes))
    syn.fill_params(head.transformer, wseed)
    with torch.no_grad():
        head.label_enc.weight.copy_(torch.from_numpy(syn.rng_normal(77, tuple(head.label_enc.weight.shape))))
        head.init_query_bbox.weight.copy_(syn.make_queries(cfg, 11)[0][0])
    return head.eval().to(DEV)


def make_inputs(cfg, seed=11):
    feats = [f.to(DEV) for f in syn.make_pyramid(cfg, seed)]
    return feats, syn.make_bev(cfg, seed, 0).to(DEV), syn.make_bev(cfg, seed, 1).to(DEV)


def run_head(head, cfg, inputs, once, metas=None):
    """-> (all_cls_scores, all_bbox_preds) of the eval head with the route on / off"""
    layer = head.transformer.decoder.decoder_layer
    layer.layer0_once = once
    feats, lss, radar = inputs
    with torch.no_grad():
        out = head(list(feats), lss, radar, [dict(m) for m in (metas or syn.make_img_metas(cfg))])
    torch.cuda.synchronize()
    layer.layer0_once = True
    return out["all_cls_scores"].clone(), out["all_bbox_preds"].clone()


def run_stages(head, cfg, inputs, once):
    """the decoder on the head's cached initial queries, under the head's key -> (cls, box, stages of layer 0)"""
    layer = head.transformer.decoder.decoder_layer
    layer.layer0_once = once
    feats, lss, radar = inputs
    stages = []
    with torch.no_grad():
        qb, qf, key = head.eval_queries(cfg.batch)
        cls, box = head.transformer(qb, qf, list(feats), lss, radar, None, syn.make_img_metas(cfg), stages_per_layer=stages,
                                    raw=True, query_key=key)
    torch.cuda.synchronize()
    layer.layer0_once = True
    return cls.clone(), box.clone(), {k: v.clone() for k, v in stages[0].items()}


@pytest.mark.parametrize("name,cfg", [("small", syn.SMALL), ("small6", syn.SMALL6), ("small_b2", replace(syn.SMALL, batch=2)),
                                      ("small6_b2", replace(syn.SMALL6, batch=2))])
def test_same_bits(name, cfg):
    head = make_head(cfg)
    layer = head.transformer.decoder.decoder_layer
    inputs = make_inputs(cfg)
    off = run_head(head, cfg, inputs, False)
    assert layer._layer0_block is None
    filled = run_head(head, cfg, inputs, True)          # fills the block
    block = layer._layer0_block
    assert block is not None and block[1]["params"].numel() == cfg.batch * cfg.num_query * layer.mixing.parameter_generator.weight.shape[0]
    hit = run_head(head, cfg, inputs, True)             # served from it
    assert layer._layer0_block is block
    for got in (filled, hit):
        assert torch.equal(got[0], off[0]) and torch.equal(got[1], off[1]), name
    s_off = run_stages(head, cfg, inputs, False)
    s_on = run_stages(head, cfg, inputs, True)
    assert layer._layer0_block is block                 # (the head's key and tensors: still the same block)
    assert torch.equal(s_on[0], s_off[0]) and torch.equal(s_on[1], s_off[1])
    for s in STAGES:
        assert torch.equal(s_on[2][s], s_off[2][s]), (name, s)
    if cfg.batch > 1:
        # different samples per batch element: the route must not make them alike
        assert not torch.equal(off[1][:, 0], off[1][:, 1])


def test_invalidation():
    cfg = syn.SMALL6
    head = make_head(cfg)
    layer = head.transformer.decoder.decoder_layer
    inputs = make_inputs(cfg)
    old = run_head(head, cfg, inputs, True)
    assert torch.equal(old[0], run_head(head, cfg, inputs, False)[0])
    for what, p in (("norm1.weight", layer.norm1.weight), ("label_enc.weight", head.label_enc.weight),
                    ("parameter_generator.weight", layer.mixing.parameter_generator.weight)):
        block = layer._layer0_block
        with torch.no_grad():
            p.mul_(1.25)
        new = run_head(head, cfg, inputs, True)
        assert layer._layer0_block is not block, what
        again = run_head(head, cfg, inputs, True)
        want = run_head(head, cfg, inputs, False)
        for got in (new, again):
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), what
        assert not torch.equal(new[0], old[0]) and not torch.equal(new[1], old[1]), what
        old = new
    # load_state_dict: a miss too
    block = layer._layer0_block
    head.load_state_dict(head.state_dict())
    run_head(head, cfg, inputs, True)
    assert layer._layer0_block is not block


def test_launch_counts():
    cfg = syn.SMALL6
    head = make_head(cfg)
    inputs = make_inputs(cfg)
    run_head(head, cfg, inputs, True)                   # fill
    names = {"sasa_fwd", "mixing_generator_gemm"}

    def count(fn):
        _lib.timer = _lib.KernelTimer(only=names)
        try:
            fn()
            torch.cuda.synchronize()
            return {k: len(v) for k, v in _lib.timer.events.items()}
        finally:
            _lib.timer = None
    assert count(lambda: run_head(head, cfg, inputs, True)) == {"sasa_fwd": 5, "mixing_generator_gemm": 5}
    assert count(lambda: run_head(head, cfg, inputs, False)) == {"sasa_fwd": 6, "mixing_generator_gemm": 6}
    # a caller without a key: random queries through the decoder
    qb, qf = (t.to(DEV) for t in syn.make_queries(cfg, 5))
    feats, lss, radar = inputs

    def no_key():
        with torch.no_grad():
            head.transformer(qb, qf, list(feats), lss, radar, None, syn.make_img_metas(cfg))
    block = head.transformer.decoder.decoder_layer._layer0_block
    assert count(no_key) == {"sasa_fwd": 6, "mixing_generator_gemm": 6}
    assert head.transformer.decoder.decoder_layer._layer0_block is block


def other_metas(cfg):
    return syn.make_img_metas(cfg, sample=3)


def test_captured_step_replays_the_shared_block():
    cfg = syn.SMALL6
    head = make_head(cfg)
    layer = head.transformer.decoder.decoder_layer
    inputs = make_inputs(cfg)
    feats, lss, radar = inputs
    metas, other = syn.make_img_metas(cfg), other_metas(cfg)
    want = run_head(head, cfg, inputs, False, metas)
    want_other = run_head(head, cfg, inputs, False, other)
    assert not torch.equal(want[1], want_other[1])
    assert layer._layer0_block is None
    caps = [CapturedStep(head, feats, lss, radar, metas, own_scratch=True) for _ in range(2)]
    block = layer._layer0_block                          # filled by the first plan's warm-up, outside capture
    assert block is not None
    ptr = block[1]["params"].data_ptr()
    for cap, ms, ref in ((caps[0], None, want), (caps[1], other, want_other), (caps[0], other, want_other), (caps[1], metas, want)):
        preds, _ = cap.replay(img_metas=ms)
        torch.cuda.synchronize()
        assert torch.equal(preds["all_cls_scores"], ref[0]) and torch.equal(preds["all_bbox_preds"], ref[1])
    assert layer._layer0_block is block and block[1]["params"].data_ptr() == ptr      # both plans read the one block
    eager = run_head(head, cfg, inputs, True, other)
    assert torch.equal(eager[0], want_other[0]) and torch.equal(eager[1], want_other[1])
    assert layer._layer0_block is block
    for cap in caps:
        cap.close()


def test_capture_with_a_cold_block_runs_the_full_layer():
    """a weight version bumped between warm-up and capture: the capture finds the block stale, must not fill it from the graph's
    pool, and replays the whole layer"""
    cfg = syn.SMALL6
    head = make_head(cfg)
    layer = head.transformer.decoder.decoder_layer
    feats, lss, radar = inputs = make_inputs(cfg)
    metas = syn.make_img_metas(cfg)
    dec = head.transformer.decoder
    staged = [dict(m) for m in metas]
    dec.stage_metas(staged, cfg.batch, torch.device(DEV))
    calls = [0]
    bias = layer.self_attn.attention.attn.out_proj.bias      # feeds the chain; no weight-derived pack is built from it

    def fn():
        calls[0] += 1
        out = head(list(feats), lss, radar, staged)
        if calls[0] == 1:
            bias.mul_(1.0)                                   # (end of the warm-up forward, outside capture)
        return out
    cap = CapturedForward(fn, torch.device(DEV), warmup=1)
    assert calls[0] == 2
    stale = layer._layer0_block
    assert stale is not None and stale[0] != layer.layer0_signature(*_key_args(head, layer, cfg, lss, radar))
    out = cap.replay()
    torch.cuda.synchronize()
    got = out["all_cls_scores"].clone(), out["all_bbox_preds"].clone()
    assert layer._layer0_block is stale                      # the capture stored nothing
    want = run_head(head, cfg, inputs, False, metas)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    out = cap.replay()
    torch.cuda.synchronize()
    assert torch.equal(out["all_bbox_preds"], want[1])


def _key_args(head, layer, cfg, lss, radar):
    with torch.no_grad():
        qb, qf, key = head.eval_queries(cfg.batch)
        return key, qb, qf, layer.prepare(lss, radar)


# ------------------------------------------------------------------------------------------------ the mixing kernels' row period
def period_fwd(x, params, period, f16x3, split):
    """rac_mixing_period_fwd called directly (mixing_fused takes rac_mixing_fwd when period == rows)"""
    B, Q, G, P, C = x.shape
    if split:
        out = torch.empty(B * Q, G * 128 * C // 32, 64, device=x.device, dtype=torch.float16)
    else:
        out = torch.empty(B, Q, G * 128 * C, device=x.device, dtype=torch.float32)
    rc = _lib.lib().rac_mixing_period_fwd(_lib.ptr(x), _lib.ptr(params), 1.0, None if split else _lib.ptr(out),
                                          _lib.ptr(out) if split else None, SPLIT_ACT_SCALE, params.stride(0), period, B * Q, G, P, C,
                                          128, 1e-5, _lib.MIX_F16X3 if f16x3 else _lib.MIX_F32, _lib.stream_ptr())
    _lib.check(rc, "rac_mixing_period_fwd")
    return out


@pytest.mark.parametrize("f16x3", [True, False], ids=["mixing_c64_f16x3_kernel", "mixing_c64_kernel"])
@pytest.mark.parametrize("P", [96, 24])
def test_mixing_row_period(P, f16x3):
    nq, G, C = 6, 4, 64
    width = G * (C * C + 128 * P)
    x = torch.from_numpy(syn.rng_normal(5, (1, nq, G, P, C))).to(DEV)
    params = torch.from_numpy(syn.rng_normal(6, (nq, width), 0.1)).to(DEV)
    for split in (False, True):
        base = mixing_fused(x, params, P, G, split=split, f16x3=f16x3)                  # rac_mixing_fwd
        assert torch.equal(period_fwd(x, params, nq, f16x3, split), base)
        half = params[:nq // 2].contiguous()
        twice = mixing_fused(x, half.repeat(2, 1), P, G, split=split, f16x3=f16x3)
        assert not torch.equal(twice, base)
        assert torch.equal(period_fwd(x, half, nq // 2, f16x3, split), twice)
        assert torch.equal(mixing_fused(x, half, P, G, split=split, f16x3=f16x3, period=nq // 2), twice)
    torch.cuda.synchronize()
