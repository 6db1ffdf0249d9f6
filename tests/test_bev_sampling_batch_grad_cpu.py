"""The BEV sampling backward for batches, without a GPU.

1. Authority of the float64 restatement tests/bev_sampling_batch_ref.py (core64_batch, written from the reference's index
   arithmetic): it agrees with BEVSampling.forward_unfused -- which carries the reference's own permute / reshape chain -- in
   float64 to 1e-9, and with the reference's own output at B = 2 (``b2:out`` of tests/golden/bev_sampling_grad_small*.npz) within
   that fixture's TOL_OUT.  Its closed-form backward is the float64 autograd of core64_batch.
2. Plumbing with float64 fakes of the two launchers at B > 1: attend_prepared(..., fused_batch=True) reproduces every ``b2:``
   gradient of the golden through _BEVSamplingCore; with the default the fused launchers are not called.
3. The argument checks of rac_bev_sampling_bwd_batch (they run before any HIP call), and that racformer_amd.fused's gate
   bev_backward_batch_fits draws the line where the library does.
4. RaCFormerTransformerDecoderLayer.forward_train asks both BEV streams for fused_batch=True."""
import ctypes

import numpy as np
import pytest
import torch

import bev_sampling_batch_ref as BB
import bev_sampling_ref as BR
from racformer_amd import _lib
from racformer_amd import fused as F
from racformer_amd import synthetic as syn
from racformer_amd import transformer as T
from test_bev_sampling_grad_cpu import (TOL_OUT, check_against_golden, fake_msda_bwd, fake_msda_fwd, inputs_from, load_golden,
                                        module_from, rel_err, t)

PC = list(syn.PC_RANGE)


@pytest.fixture
def fake_msda(monkeypatch):
    monkeypatch.setattr(T, "msda_forward", fake_msda_fwd)
    monkeypatch.setattr(T, "msda_backward", fake_msda_bwd)


@pytest.fixture
def batch_fakes(monkeypatch):
    monkeypatch.setattr(T, "bev_sampling_fused", BB.fake_fused_batch)
    monkeypatch.setattr(T, "bev_sampling_backward", BB.fake_backward_batch)
    BR.CALLS.clear()


def case(seed, B, Tn, Q, heads, NP, D, H, W, outside=False, dtype=np.float64, d_lo=0.05):
    """a random kernel-level case of batch B (float64 by default; the GPU tests draw theirs in float32).  ``d_lo``: the smallest
    query radius, as a fraction of 65 m"""
    rng = np.random.default_rng(seed)
    P = NP * D
    qb = rng.random((B, Q, 10)).astype(dtype)
    qb[..., 1] = d_lo + (0.6 - d_lo) * qb[..., 1]
    if outside:
        qb[:, ::2, 1] = 1.3                                     # far outside the map: clamped keypoints
    qb[..., 6:8] = qb[..., 6:8] * 2 - 1
    qb[..., 8:10] = qb[..., 8:10] * 4 - 2
    c = dict(value=t(rng.standard_normal((B * Tn, H * W, heads, 64)).astype(dtype)), hw=(H, W), query_bbox=t(qb),
             off=t(rng.uniform(-1.5, 1.5, (B, Q, heads * P * 2)).astype(dtype)), ray=t(rng.standard_normal((B, Q, D)).astype(dtype)),
             sc=t(rng.standard_normal((B, Q, heads * P)).astype(dtype)), qu=t(rng.standard_normal((B, Q, Tn)).astype(dtype)),
             time_diff=t((rng.random((B, Tn)) * 0.1 + np.arange(Tn) * 0.5).astype(dtype)), T=Tn, heads=heads, NP=NP, D=D, pc=PC, d_region=0.1)
    return c, t(rng.standard_normal((B, Q, heads * 64)).astype(dtype))


# ------------------------------------------------------------------------------------------------------------- 1. authority
def test_restatement_agrees_with_forward_unfused_in_float64(golden_dir, fake_msda):
    """the module's own torch chain (keypoints, the MSDA operator restated by the oracle, attend's permutes and frame fusion) in
    float64 on the golden's B = 2 inputs, against core64_batch + output_proj + identity: 1e-9 of the largest element"""
    g = load_golden(golden_dir)
    m = module_from(g, dtype=torch.float64, requires_grad=False)
    qr, qf, bev, metas, _ = inputs_from(g, "b2:", dtype=torch.float64)
    d_region = float(g["d_region"])
    with torch.no_grad():
        value, hw = m.prepare_value(bev)
        want = m.forward_unfused(qr, qf, value, hw, metas[0]["time_diff"], d_region)
        lin = [mod(qf) for mod in (m.sampling_offset, m.ray_points_offset, m.scale_weights, m.attention.bev_queue_weight)]
        # (the module's float64 chain forms the depth bases in float64, the launcher in float32: hand the module's to the restatement)
        dbase = torch.linspace(-d_region, d_region, m.depth_num, dtype=torch.float64)
        core, _ = BB.core64_batch(value, hw, qr, *lin, metas[0]["time_diff"], m.num_frames, m.num_heads, m.num_points, m.depth_num,
                                  m.pc_range, d_region, dbase=dbase)
        got = m.attention.output_proj(core) + qf
        undone, _ = BB.core64_batch(value, hw, qr, *lin, metas[0]["time_diff"], m.num_frames, m.num_heads, m.num_points, m.depth_num,
                                    m.pc_range, d_region, dbase=dbase, paired=False)
    assert qr.shape[0] == 2 and rel_err(got, want.numpy()) < 1e-9
    # the pairing matters on this input: undone, the restatement is nowhere near
    assert rel_err(m.attention.output_proj(undone) + qf, want.numpy()) > 1e-3


def test_restatement_agrees_with_the_reference_output_b2(golden_dir):
    g = load_golden(golden_dir)
    m = module_from(g, dtype=torch.float64, requires_grad=False)
    qr, qf, bev, metas, _ = inputs_from(g, "b2:", dtype=torch.float64)
    with torch.no_grad():
        value, hw = m.prepare_value(bev)
        lin = [mod(qf) for mod in (m.sampling_offset, m.ray_points_offset, m.scale_weights, m.attention.bev_queue_weight)]
        core, _ = BB.core64_batch(value, hw, qr, *lin, metas[0]["time_diff"], m.num_frames, m.num_heads, m.num_points, m.depth_num,
                                  m.pc_range, float(g["d_region"]))
        got = m.attention.output_proj(core) + qf
    assert rel_err(got, g["b2:out"]) < TOL_OUT


@pytest.mark.parametrize("shape", [(2, 3, 5, 4, 2, 5, 12, 10, False), (3, 4, 4, 1, 1, 3, 8, 8, False), (4, 2, 6, 3, 2, 2, 9, 7, True),
                                   (1, 3, 5, 4, 2, 5, 12, 10, False)])
def test_closed_form_backward_is_the_autograd_of_the_restatement(shape):
    *dims, outside = shape
    B, Tn, Q, heads, NP, D, H, W = dims
    c, gout = case(sum(dims), *dims, outside=outside)
    got = BB.closed_form_bwd_batch(gout=gout, **c)
    leaves = {k: c[k].clone().requires_grad_() for k in ("value", "off", "ray", "sc", "qu")}
    table = T.box_table_torch(c["query_bbox"], PC).requires_grad_()
    out, loc = BB.core64_batch(**{**c, **leaves}, box_table=table)
    loc.retain_grad()
    (out * gout).sum().backward()
    want = dict(grad_value=leaves["value"].grad, grad_offsets=leaves["off"].grad, grad_ray=leaves["ray"].grad,
                grad_scale=leaves["sc"].grad, grad_queue=leaves["qu"].grad, grad_box=table.grad, grad_loc=loc.grad)
    if outside:
        assert bool(((loc == 0) | (loc == 1)).any())
    for k, w_ in want.items():
        assert got[k].shape == w_.shape, k
        assert (got[k] - w_).abs().max().item() < 1e-11 * max(1.0, w_.abs().max().item()), k
    if B == 1:      # one sample: the restatement of tests/bev_sampling_ref.py
        old = BR.closed_form_bwd(gout=gout, **c)
        for k in want:
            assert (got[k].reshape(old[k].shape) - old[k]).abs().max().item() < 1e-12 * max(1.0, old[k].abs().max().item()), k


# -------------------------------------------------------------------------------------------------------------- 2. plumbing
def test_fused_batch_reproduces_the_reference_gradients_b2(golden_dir, batch_fakes):
    g = load_golden(golden_dir)
    m = module_from(g)
    qr, qf, bev, metas, gout = inputs_from(g, "b2:")
    value, hw = m.prepare_value(bev)
    out = m.attend_prepared(qr, qf, value, hw, metas[0]["time_diff"], float(g["d_region"]), fused_batch=True)
    (out * gout).sum().backward()
    assert [c_[0] for c_ in BR.CALLS] == ["fwd", "bwd"]
    assert BR.CALLS[0][3] == (2, 21, 10) and BR.CALLS[1][1] == (2, 21, 256)
    check_against_golden(g, "b2:", m, qr, qf, bev, out)


def test_default_route_at_b2_stays_unfused(golden_dir, batch_fakes, fake_msda):
    g = load_golden(golden_dir)
    m = module_from(g)
    qr, qf, bev, metas, gout = inputs_from(g, "b2:")
    value, hw = m.prepare_value(bev)
    out = m.attend_prepared(qr, qf, value, hw, metas[0]["time_diff"], float(g["d_region"]))
    (out * gout).sum().backward()
    assert BR.CALLS == []
    out = m(qr, qf, bev, metas, d_region=float(g["d_region"]))           # BEVSampling.forward keeps the default
    assert BR.CALLS == [] and out.grad_fn is not None


def test_a_batch_beyond_the_lds_takes_the_unfused_route(golden_dir, batch_fakes, fake_msda, monkeypatch):
    """fused_batch=True where the launcher would refuse B: forward_unfused, not an error"""
    g = load_golden(golden_dir)
    m = module_from(g)
    qr, qf, bev, metas, _ = inputs_from(g, "b2:")
    value, hw = m.prepare_value(bev)
    monkeypatch.setattr(T, "bev_backward_batch_fits", lambda *a: False)
    out = m.attend_prepared(qr, qf, value, hw, metas[0]["time_diff"], float(g["d_region"]), fused_batch=True)
    assert BR.CALLS == [] and out.grad_fn is not None


# ------------------------------------------------------------------------------------------------------ 3. argument checks
def _lib_or_fail():
    try:
        return _lib.lib()
    except RuntimeError as e:
        pytest.fail(str(e))


def _bwd_batch(lib, B=2, Tn=3, Q=21, heads=4, NP=2, D=5, H=12, W=10, dim=64, dtype=_lib.RAC_F32, ld=(80, 5, 40, 3), gld=(80, 5, 40, 3),
               ptr=ctypes.c_void_p(16), gv=ctypes.c_void_p(16), host=True):
    pc = (ctypes.c_float * 6)(*syn.PC_RANGE)
    db = (ctypes.c_float * 5)(-0.1, -0.05, 0.0, 0.05, 0.1)
    return lib.rac_bev_sampling_bwd_batch(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, gv, ptr, ptr, ptr, ptr, ptr, None, None,
                                          *ld, *gld, B, Tn, Q, heads, NP, D, H, W, dim, pc if host else None, db if host else None,
                                          0.1, dtype, None)


def test_bev_sampling_bwd_batch_argument_errors():
    """never-dereferenced pointers: every call below fails its checks first"""
    lib = _lib_or_fail()

    def last():
        msg = lib.rac_last_error().decode()
        assert "rac_bev_sampling_bwd_batch" in msg, msg
        return msg

    bwd = lambda **kw: _bwd_batch(lib, **kw)  # noqa: E731
    assert bwd(B=0) == -1 and "bad sizes" in last() and "B=0" in last()
    assert bwd(B=-1) == -1 and "bad sizes" in last()
    assert bwd(B=4096) == -1 and "LDS" in last() and "B=4096" in last()
    assert bwd(dtype=_lib.RAC_BF16) == -1 and "dtype 1" in last()
    assert bwd(dtype=_lib.RAC_I16) == -1 and "dtype 2" in last()
    assert bwd(dim=32) == -1 and "dim=32" in last()
    assert bwd(D=17) == -1 and "bad sizes" in last()
    assert bwd(Tn=0) == -1 and "bad sizes" in last()
    assert bwd(Tn=65) == -1 and "max 64" in last()
    assert bwd(NP=13) == -1 and "max 64" in last()                        # 13 * 5 points
    assert bwd(ld=(79, 5, 40, 3)) == -1 and "row strides" in last()
    assert bwd(ld=(80, 5, 40, 2)) == -1 and "row strides" in last()
    assert bwd(gld=(80, 4, 40, 3)) == -1 and "gradient row strides" in last()
    assert bwd(gld=(80, 5, 39, 3)) == -1 and "gradient row strides" in last()
    assert bwd(B=1, heads=16, Tn=64, NP=2, D=5, ld=(320, 5, 160, 64), gld=(320, 5, 160, 64)) == -1 and "LDS" in last()
    assert bwd(ptr=None) == -1 and "null pointer" in last()
    assert bwd(gv=None) == -1 and "null pointer" in last()
    assert bwd(host=False) == -1 and "null pointer" in last()
    assert bwd(Q=0, ptr=None, gv=None) == 0                               # empty: nothing to check or launch
    # the old symbol keeps refusing a batch
    d = ctypes.c_void_p(16)
    pc = (ctypes.c_float * 6)(*syn.PC_RANGE)
    db = (ctypes.c_float * 5)(-0.1, -0.05, 0.0, 0.05, 0.1)
    assert lib.rac_bev_sampling_bwd(d, d, d, d, d, d, d, d, d, d, d, d, d, d, d, None, None, 80, 5, 40, 3, 80, 5, 40, 3, 2, 3, 21, 4, 2, 5,
                                    12, 10, 64, pc, db, 0.1, _lib.RAC_F32, None) == -1
    assert "B == 1 only" in lib.rac_last_error().decode()


@pytest.mark.parametrize("shape", [(4, 8, 4, 5), (4, 3, 2, 5), (1, 2, 1, 3), (8, 16, 4, 5)])
def test_python_gate_draws_the_line_where_the_library_does(shape):
    """the largest B bev_backward_batch_fits accepts passes the library's LDS check (and fails the next one: the null pointers);
    B + 1 is refused for its LDS"""
    lib = _lib_or_fail()
    heads, Tn, NP, D = shape
    P = NP * D
    B = max(b for b in range(1, 4096) if F.bev_backward_batch_fits(b, heads, Tn, P))
    ld = (heads * P * 2, D, heads * P, Tn)
    kw = dict(Tn=Tn, heads=heads, NP=NP, D=D, ld=ld, gld=ld, ptr=None, gv=None)
    assert _bwd_batch(lib, B=B, **kw) == -1 and "null pointer" in lib.rac_last_error().decode()
    assert _bwd_batch(lib, B=B + 1, **kw) == -1 and "LDS" in lib.rac_last_error().decode()
    assert not F.bev_backward_batch_fits(0, heads, Tn, P)


# ------------------------------------------------------------------------------------------------------- 4. the training route
def test_forward_train_asks_both_streams_for_the_fused_batch(monkeypatch):
    """forward_train on a tiny CPU rig at B = 2, every heavy module replaced by a stand-in: both BEV samplings are called with
    fused_batch=True and the layer's own box table"""
    import decoder_grad_ref as DR
    from racformer_amd.transformer import RaCFormerTransformerDecoderLayer
    torch.manual_seed(0)
    layer = RaCFormerTransformerDecoderLayer(**DR.LAYER_KW).eval()
    B, Q, E = 2, 5, DR.E
    seen = []

    def bev_stub(name):
        def attend(query_ray, query_feat, value, hw, time_diff, d_region, linear_out=None, box_table=None, **kw):
            seen.append((name, kw, tuple(query_ray.shape), tuple(time_diff.shape), box_table is not None, len(linear_out)))
            return query_feat + linear_out[3].sum(-1, keepdim=True)
        return attend

    monkeypatch.setattr(layer.sampling_radar_bev, "attend_prepared", bev_stub("radar"))
    monkeypatch.setattr(layer.sampling_lss_bev, "attend_prepared", bev_stub("lss"))
    monkeypatch.setattr(layer.self_attn, "forward", lambda qb, qf, mask, w: qf)
    monkeypatch.setattr(layer, "_sample", lambda qb, qf, *a: qf[:, :, None, None, :64].expand(B, Q, 4, 2, 64))
    monkeypatch.setattr(layer.mixing, "forward", lambda s, qf, w: qf + s.sum((2, 3)).repeat(1, 1, 4))
    monkeypatch.setattr(T, "box_prep", lambda qb, pc: T.box_table_torch(qb.detach(), pc))
    monkeypatch.setattr(T, "_RefineCore", type("R", (), {"apply": staticmethod(lambda qb, delta, td, n: (qb + delta, qb + delta))}))
    qb = torch.rand(B, Q, 10).requires_grad_()
    qf = torch.randn(B, Q, E).requires_grad_()
    td = torch.arange(DR.T, dtype=torch.float32)[None].repeat(B, 1) * 0.5
    w, b_, widths = layer._wide_linears()
    prepared = dict(radar_value=None, radar_hw=DR.BEV_HW, lss_value=None, lss_hw=DR.BEV_HW, wide_w=w, wide_b=b_, wide_widths=widths)
    feat, cls, pred = layer.forward_train(qb, qf, [], None, [dict(time_diff=td, time_diff_safe=td + 1)], DR.LAYER, prepared)
    assert [(s[0], s[1]) for s in seen] == [("radar", dict(fused_batch=True)), ("lss", dict(fused_batch=True))]
    assert all(s[2] == (B, Q, 10) and s[3] == (B, DR.T) and s[4] and s[5] == 4 for s in seen)
    (feat.sum() + cls.sum()).backward()
    assert qf.grad is not None and layer.sampling_lss_bev.attention.bev_queue_weight.weight.grad is not None
