"""The split-precision route of AdaptiveMixing's two big Linears under autograd, without a GPU.

The four launch sequences (split_generator_forward / _backward, split_outproj_forward / _backward) and the mixing core's two
launchers are replaced HERE by float64 torch restatements that behave like the real ones: plain tensors in and out, no autograd
history.  What is checked is the host-side plumbing: _SplitLinearCore, the switch AdaptiveMixing.fused_linear_grad, the fallbacks
(switch off, shapes outside the kernels' limits, weights f16 cannot hold, no gradient wanted), that AdaptiveMixing.forward is not
rerouted, the pack cache's key, the wrappers' refusal of host tensors and the C entry points' argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from racformer_amd import _lib
from racformer_amd import fused as Fz
from racformer_amd import transformer as T
from mixing_ref import closed_form_bwd, core64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = []
TOL_OUT, TOL_GRAD = 2e-6, 1e-5     # (the figures of tests/test_mixing_grad_cpu.py: float64 restatements against a float32 reference)


def t(a):
    return torch.from_numpy(np.asarray(a)).clone()


class FakePacks(dict):
    def __init__(self, gen_w, out_w):
        super().__init__(gen=gen_w.detach(), out=out_w.detach())


def fake_gen_fwd(query, packs, bias):
    CALLS.append("gen_fwd")
    with torch.no_grad():
        return (query.double() @ packs["gen"].double().t() + bias.double()).float(), query.abs().max().reshape(1)


def fake_gen_bwd(query, amax, gp, packs, need_q, need_w, need_b):
    CALLS.append(("gen_bwd", need_q, need_w, need_b, gp.is_contiguous()))
    with torch.no_grad():
        g = gp.double()
        return ((g @ packs["gen"].double()).float() if need_q else None, (g.t() @ query.double()).float() if need_w else None,
                g.sum(0).float() if need_b else None)


def fake_out_fwd(z, packs, bias):
    CALLS.append("out_fwd")
    with torch.no_grad():
        return (z.double() @ packs["out"].double().t() + bias.double()).float(), z.abs().max().reshape(1)


def fake_out_bwd(z, amax, g, packs, need_z, need_w, need_b):
    CALLS.append(("out_bwd", need_z, need_w, need_b, g.is_contiguous()))
    with torch.no_grad():
        g = g.double()
        return ((g @ packs["out"].double()).float() if need_z else None, (g.t() @ z.double()).float() if need_w else None,
                g.sum(0).float() if need_b else None)


def fake_fused(x, params, in_points, n_groups, out_points=128, eps=1e-5, split=False, param_scale=1.0, f16x3=False, out=None):
    CALLS.append("mix_fwd")
    with torch.no_grad():
        return core64(x, params, in_points, n_groups).float()


def fake_backward(x, params, grad_out, in_points, n_groups, out_points=128, eps=1e-5, grad_x=None, grad_params=None, z_out=None):
    CALLS.append("mix_bwd")
    with torch.no_grad():
        gx, gp = closed_form_bwd(x, params, grad_out, in_points, n_groups)
    return gx.float(), gp.float()


@pytest.fixture
def fakes(monkeypatch):
    for name, fn in [("split_generator_forward", fake_gen_fwd), ("split_generator_backward", fake_gen_bwd),
                     ("split_outproj_forward", fake_out_fwd), ("split_outproj_backward", fake_out_bwd),
                     ("mixing_fused", fake_fused), ("mixing_backward", fake_backward), ("LinearGradPacks", FakePacks)]:
        monkeypatch.setattr(T, name, fn)
    monkeypatch.setattr(T.AdaptiveMixing, "fused_supported", lambda self, x: True)
    monkeypatch.setattr(FakePacks, "complete", lambda self: bool((self["gen"] != 0).any()) and bool((self["out"] != 0).any()), raising=False)
    monkeypatch.setattr(T.AdaptiveMixing, "fused_linear_grad", True)
    CALLS.clear()


def _pad_last(a, n=256):
    return torch.cat([a, a.new_zeros(a.shape[:-1] + (n - a.shape[-1],))], dim=-1)


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "mixing_grad_small.npz"))


def _embedded(g, requires_grad=True):
    """the fixture (query_dim 4) embedded exactly in query_dim 256: zero-padded query columns, weight columns / rows and bias"""
    P, G = int(g["in_points"]), int(g["n_groups"])
    m = T.AdaptiveMixing(in_dim=64 * G, in_points=P, n_groups=G, query_dim=256, out_points=128).eval()
    m.load_state_dict({"parameter_generator.weight": _pad_last(t(g["w:parameter_generator.weight"]).float()),
                       "parameter_generator.bias": t(g["w:parameter_generator.bias"]).float(),
                       "out_proj.weight": _pad_last(t(g["w:out_proj.weight"]).float().t()).t().contiguous(),
                       "out_proj.bias": _pad_last(t(g["w:out_proj.bias"]).float())})
    for p in m.parameters():
        p.requires_grad_(requires_grad)
    return m


def _rel_err(got, want):
    want = t(want).double()
    return ((got.detach().double() - want).abs().max() / want.abs().max()).item()


def test_switch_on_takes_the_split_route_and_matches_the_reference(golden_dir, fakes):
    g = _golden(golden_dir)
    QD = g["query"].shape[-1]
    m = _embedded(g)
    x = t(g["x"]).requires_grad_()
    query = _pad_last(t(g["query"])).requires_grad_()
    out = m.forward_train(x, query)
    assert CALLS == ["gen_fwd", "mix_fwd", "out_fwd"]
    assert _rel_err(out[..., :QD], g["out"]) < TOL_OUT
    (out * _pad_last(t(g["gout"]))).sum().backward()
    assert CALLS[3:] == [("out_bwd", True, True, True, True), "mix_bwd", ("gen_bwd", True, True, True, True)]
    p = dict(m.named_parameters())
    got = {"x": x.grad, "query": query.grad[..., :QD], "parameter_generator.weight": p["parameter_generator.weight"].grad[:, :QD],
           "parameter_generator.bias": p["parameter_generator.bias"].grad, "out_proj.weight": p["out_proj.weight"].grad[:QD],
           "out_proj.bias": p["out_proj.bias"].grad[:QD]}
    for k, v in got.items():
        assert v is not None, k
        assert _rel_err(v, g["g:" + k]) < TOL_GRAD, k


def test_gradients_not_asked_for_are_not_computed(golden_dir, fakes):
    g = _golden(golden_dir)
    m = _embedded(g, requires_grad=False)
    x = t(g["x"]).requires_grad_()
    query = _pad_last(t(g["query"])).requires_grad_()
    (m.forward_train(x, query) * _pad_last(t(g["gout"]))).sum().backward()
    assert ("out_bwd", True, False, False, True) in CALLS and ("gen_bwd", True, False, False, True) in CALLS
    assert all(p.grad is None for p in m.parameters()) and x.grad is not None and query.grad is not None
    CALLS.clear()
    m = _embedded(g)
    (m.forward_train(t(g["x"]), _pad_last(t(g["query"]))) * _pad_last(t(g["gout"]))).sum().backward()
    # inputs without grad: no data gradient of the generator; out_proj's is still wanted, by the generated parameters
    assert ("gen_bwd", False, True, True, True) in CALLS and ("out_bwd", True, True, True, True) in CALLS


def _spy_forward(monkeypatch):
    seen = []
    real = T.AdaptiveMixing.forward

    def forward(self, x, query, out_proj_split=None):
        seen.append(out_proj_split is not None)
        return real(self, x, query, out_proj_split)

    monkeypatch.setattr(T.AdaptiveMixing, "forward", forward)
    return seen


def _split_calls():
    return [c for c in CALLS if c in ("gen_fwd", "out_fwd")]


def test_fallbacks_take_the_route_of_before(golden_dir, fakes, monkeypatch):
    g = _golden(golden_dir)
    seen = _spy_forward(monkeypatch)
    x, query = t(g["x"]).requires_grad_(), _pad_last(t(g["query"])).requires_grad_()
    m = _embedded(g)
    # the switch off (the class attribute or an instance's)
    m.fused_linear_grad = False
    out = m.forward_train(x, query)
    assert seen == [True] and not _split_calls() and out.grad_fn is not None     # (the split operand is built for forward)
    del m.fused_linear_grad
    # no gradient wanted: no_grad, and grad mode with nothing that requires grad
    with torch.no_grad():
        m.forward_train(x, query)
    _embedded(g, requires_grad=False).forward_train(x.detach(), query.detach())
    assert seen == [True] * 3 and not _split_calls()
    # weights f16 cannot hold: the packs give up (here: an all-zero generator weight, the model's own initialisation)
    z = _embedded(g)
    with torch.no_grad():
        z.parameter_generator.weight.zero_()
    assert z.linear_grad_packs() is None
    z.forward_train(x, query)
    assert seen == [True] * 4 and not _split_calls()
    # a shape outside the kernels' limits: the fixture's own query_dim, 4
    P, G = int(g["in_points"]), int(g["n_groups"])
    small = T.AdaptiveMixing(in_dim=64 * G, in_points=P, n_groups=G, query_dim=4, out_points=128).eval()
    q4 = t(g["query"]).requires_grad_()
    assert not small.linear_grad_supported(x, q4)
    small.forward_train(x, q4)
    assert seen == [True] * 5 and not _split_calls()
    # and the route itself, for contrast
    m.forward_train(x, query)
    assert seen == [True] * 5 and _split_calls() == ["gen_fwd", "out_fwd"]


def test_forward_is_not_rerouted_by_the_switch(golden_dir, fakes):
    g = _golden(golden_dir)
    m = _embedded(g)
    x, query = t(g["x"]).requires_grad_(), _pad_last(t(g["query"])).requires_grad_()
    out = m(x, query, m.split_out_proj())
    out.sum().backward()
    assert CALLS == ["mix_fwd", "mix_bwd"]


def test_packs_are_cached_on_the_weight_versions(golden_dir, fakes):
    g = _golden(golden_dir)
    m = _embedded(g)
    a = m.linear_grad_packs()
    assert m.linear_grad_packs() is a
    with torch.no_grad():
        m.out_proj.weight.mul_(2.0)             # what an optimiser step does: an in-place update bumps _version
    b = m.linear_grad_packs()
    assert b is not a and torch.equal(b["out"], m.out_proj.weight.detach())
    assert not hasattr(m, "_pack_cache")


def test_decoder_layer_uses_the_route_only_on_the_training_path():
    import inspect
    src = inspect.getsource(T.RaCFormerTransformerDecoderLayer)
    assert src.count("mixing.forward_train(") == 1 and "mixing.forward_train(" in inspect.getsource(T.RaCFormerTransformerDecoderLayer.forward_train)
    assert "fused_linear_grad" not in inspect.getsource(T.AdaptiveMixing.forward)


def test_wrappers_raise_on_host_tensors():
    v, a = torch.zeros(4, 256), torch.zeros(1)
    img = torch.zeros(4, 8, 64, dtype=torch.float16)
    for fn in (lambda: Fz.absmax_device(v), lambda: Fz.linear_pack_act(v, a), lambda: Fz.pack_linear_weight_t(v),
               lambda: Fz.generator_ds(img, img, None, 1.0, a), lambda: Fz.linear_reduce(torch.zeros(2, 4, 256), None, a, 1.0),
               lambda: Fz.linear_wgrad(img, a, v, a, False)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn()


def test_outproj_slices_divide_the_reduction():
    for K, want in [(32768, 32), (65536, 64), (4608, 4), (19968, 16), (8192, 8), (128, 1), (384, 1)]:
        s = Fz.outproj_slices(K)
        assert s == want and K % (32 * s) == 0


def _lib_or_fail():
    try:
        return _lib.lib()
    except RuntimeError as e:
        pytest.fail(str(e))


def test_c_entry_points_refuse_other_shapes():
    lib = _lib_or_fail()
    d = ctypes.c_void_p(16)      # never dereferenced: every call below fails its checks first
    last = lambda: lib.rac_last_error().decode()  # noqa: E731
    assert lib.rac_linear_wgrad(d, d, d, 128, d, d, None, 5, 128, 128, 0, None) == -1 and "narrow side of 256" in last()
    assert lib.rac_linear_wgrad(d, d, d, 192, d, d, None, 5, 256, 192, 0, None) == -1 and "multiple of 128" in last()
    assert lib.rac_linear_wgrad(d, d, d, 130, d, d, None, 5, 256, 128, 0, None) == -1 and "ld_wide" in last()
    assert lib.rac_linear_wgrad(d, d, ctypes.c_void_p(20), 128, d, d, None, 5, 256, 128, 0, None) == -1 and "16-byte aligned" in last()
    assert lib.rac_linear_wgrad(d, d, d, 128, d, d, None, 0, 256, 128, 0, None) == -1
    assert lib.rac_linear_pack_act(d, 30, d, d, 5, 32, None) == -1 and "ld_src" in last()
    assert lib.rac_linear_pack_wt(d, d, 48, 64, 1.0, None) == -1 and "multiples of 32" in last()
    assert lib.rac_generator_ds_fwd(d, d, None, 1.0, d, d, 128, 5, 128, 64, None) == -1 and "K = 256" in last()
    assert lib.rac_linear_reduce(d, None, d, 1.0, d, 6, 2, 5, 6, None) == -1 and "multiples of 4" in last()


def test_header_declares_the_new_entry_points_and_abi():
    h = open(os.path.join(ROOT, "include", "racformer_hip.h")).read()
    assert int(re.search(r"#define\s+RAC_ABI_VERSION\s+(\d+)", h).group(1)) >= 22
    for name in ("rac_linear_pack_act", "rac_linear_pack_wt", "rac_generator_ds_fwd", "rac_linear_reduce", "rac_linear_wgrad"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", h), name
        assert name in _lib.SIGNATURES
        assert hasattr(_lib_or_fail(), name)
