"""Autograd through RaCFormerSampling's fused path without a GPU.

The two HIP launchers (sampling4d_fused, sampling4d_backward) are replaced HERE by the float64 torch fakes of
tests/sampling4d_core_ref.py, which behave like the real ones: plain tensors in and out, no autograd history, the backward
writing into the destinations it is handed.  What is checked is the host-side plumbing around them -- the three Linears, the
box table as a differentiable input, the routing by autograd state -- against the reference's own autograd
(tests/golden/racsampling_grad_small.npz, gen_golden_racsampling_grad.py).  Also the closed-form backward the kernel
implements against float64 autograd of the restated forward, and the argument checks of rac_sampling4d_bwd, which run
before any HIP call."""
import ctypes
import os

import numpy as np
import pytest
import torch

import sampling4d_core_ref as SR
from racformer_amd import _lib
from racformer_amd import synthetic as syn
from racformer_amd import transformer as T

E = 256
# Same kind of comparison as test_bev_sampling_grad_cpu.py: max |err| / max |value| per tensor, 1e-5 for the gradients.  The
# reference runs in float32 and the fakes in float64, so what is measured here is the float32 reference's own rounding: through
# the polar round trip at up to 42 m and the projection it comes to 6.1e-6 of the output's largest element and up to 7.2e-6 of a
# gradient's (measured at the fixture's seed), hence 1e-5 for the output too.  (The GPU test of the module keeps 5e-6 for it.)
TOL_OUT, TOL_GRAD = 1e-5, 1e-5


def t(a):
    return torch.from_numpy(np.asarray(a)).clone()


def load_golden(golden_dir):
    with np.load(os.path.join(golden_dir, "racsampling_grad_small.npz")) as z:
        return {k: z[k] for k in z.files}


def module_from(g, dtype=torch.float32, requires_grad=True):
    G, Tn, NP, D, N, L = (int(x) for x in g["shape"])
    m = T.RaCFormerSampling(embed_dims=E, num_frames=Tn, num_groups=G, num_points=NP, num_levels=L, depth_num=D,
                            pc_range=list(syn.PC_RANGE)).eval()
    m.load_state_dict({k[2:]: t(v).float() for k, v in g.items() if k.startswith("w:")})
    m = m.to(dtype)
    for p in m.parameters():
        p.requires_grad_(requires_grad)
    return m


def inputs_from(g, dtype=torch.float32, device="cpu"):
    L = int(g["shape"][5])
    qr, qf = (t(g[k]).to(dtype).to(device).requires_grad_() for k in ("query_ray", "query_feat"))
    feats = [t(g[f"feat{i}"]).to(dtype).to(device).requires_grad_() for i in range(L)]
    h, w = (int(x) for x in g["image_hw"])
    metas = [dict(img_shape=[(h, w, 3)], time_diff=t(g["time_diff"]).to(dtype).to(device), lidar2img=t(g["lidar2img"]).to(dtype).to(device))]
    return qr, qf, feats, metas, t(g["gout"]).to(dtype).to(device)


def rel_err(got, want):
    want = t(want).double()
    return ((got.detach().cpu().double() - want).abs().max() / want.abs().max()).item()


def check_against_golden(g, m, qr, qf, feats, out, tol_out=TOL_OUT, tol_grad=TOL_GRAD):
    assert rel_err(out, g["out"]) < tol_out
    worst = {}
    for name, got in [("query_feat", qf.grad), ("query_ray", qr.grad)] + [(f"feat{i}", f.grad) for i, f in enumerate(feats)] + \
            [(k, p.grad) for k, p in m.named_parameters()]:
        assert got is not None, f"{name}: no gradient"
        worst[name] = rel_err(got, g["g:" + name])
    print("\n" + "\n".join(f"  {k:>40s}: {v:.2e}" for k, v in worst.items()))
    bad = {k: v for k, v in worst.items() if not v < tol_grad}
    assert not bad, bad
    gq = qr.grad
    assert float(gq[..., [8, 9]].abs().max()) == 0.0 and all(float(gq[..., i].abs().max()) > 0 for i in range(8))


@pytest.fixture
def fakes(monkeypatch):
    monkeypatch.setattr(T, "sampling4d_fused", SR.fake_fused)
    monkeypatch.setattr(T, "sampling4d_backward", SR.fake_backward)
    SR.CALLS.clear()


def test_module_gradients_match_the_reference(golden_dir, fakes):
    """every key of the golden through _Sampling4DCore; fails where the fused path has no autograd history"""
    g = load_golden(golden_dir)
    m = module_from(g)
    qr, qf, feats, metas, gout = inputs_from(g)
    out = m(qr, qf, feats, metas, d_region=float(g["d_region"]))
    assert out.grad_fn is not None
    (out * gout).sum().backward()
    assert [c[0] for c in SR.CALLS] == ["fwd", "bwd"]
    assert SR.CALLS[1] == ("bwd", tuple(gout.shape), True, False, False, True)
    check_against_golden(g, m, qr, qf, feats, out)


def test_caller_table_linear_out_and_debug(golden_dir, fakes):
    """the decoder layer's way of calling: Linear outputs as column slices of one wide GEMM output, its own box table; the debug
    outputs come back without autograd history; frozen features ask for no feature gradient"""
    g = load_golden(golden_dir)
    m = module_from(g)
    qr, qf, feats, metas, gout = inputs_from(g)
    feats = [f.detach() for f in feats]
    mods = [m.sampling_offset, m.ray_points_offset, m.scale_weights]
    wide = torch.nn.functional.linear(qf, torch.cat([x.weight for x in mods]), torch.cat([x.bias for x in mods]))
    lin = wide.split([x.weight.shape[0] for x in mods], dim=-1)
    table = T.box_table_torch(qr.detach(), m.pc_range)
    m.capture_loc = []
    out, loc, w = m(qr, qf, feats, metas, d_region=float(g["d_region"]), linear_out=lin, box_table=table, debug=True)
    assert out.grad_fn is not None and not loc.requires_grad and not w.requires_grad and m.capture_loc[0] is loc
    (out * gout).sum().backward()
    assert SR.CALLS[0][15:18] == (True, True, False) and SR.CALLS[1] == ("bwd", tuple(gout.shape), True, True, False, False)
    assert rel_err(out, g["out"]) < TOL_OUT
    for name, got in (("query_feat", qf.grad), ("query_ray", qr.grad)):
        assert rel_err(got, g["g:" + name]) < TOL_GRAD, name


def test_no_grad_and_frozen_launch_what_they_launched_before(golden_dir, fakes):
    """under no_grad / inference_mode, and in grad mode with nothing requiring grad: one plain forward launch with today's arguments"""
    g = load_golden(golden_dir)
    m = module_from(g)
    qr, qf, feats, metas, _ = inputs_from(g)
    d_region = float(g["d_region"])
    with torch.no_grad():
        a = m(qr, qf, feats, metas, d_region=d_region)
    with torch.inference_mode():
        b = m(qr, qf, feats, metas, d_region=d_region)
    c = module_from(g, requires_grad=False)(qr.detach(), qf.detach(), [f.detach() for f in feats], metas, d_region=d_region)
    G, Tn, NP, D, N, L = (int(x) for x in g["shape"])
    P = NP * D
    h, w = (int(x) for x in g["image_hw"])
    want = ("fwd", L, tuple(feats[0].shape), (1, 21, 10), G * P * 3, D, G * Tn * P * L, Tn, G, NP, D, d_region, float(h), float(w), 1e-5,
            False, False, False, None)
    assert SR.CALLS == [want] * 3
    for o in (a, b, c):
        assert o.grad_fn is None and not o.requires_grad and rel_err(o, g["out"]) < TOL_OUT


def test_imposed_views_reach_both_launches(golden_dir, fakes):
    g = load_golden(golden_dir)
    m = module_from(g)
    qr, qf, feats, metas, gout = inputs_from(g)
    G, Tn, NP, D, N, L = (int(x) for x in g["shape"])
    m.force_views = [torch.ones(Tn * G, 21, NP * D, dtype=torch.uint8)]
    out = m(qr, qf, feats, metas, d_region=float(g["d_region"]))
    (out * gout).sum().backward()
    assert SR.CALLS[0][17] is True and SR.CALLS[1][4] is True and m.force_views == []


def test_bf16_features_raise_at_backward_time(golden_dir, fakes):
    g = load_golden(golden_dir)
    m = module_from(g)
    qr, qf, feats, metas, gout = inputs_from(g)
    out = m(qr, qf, [f.detach().bfloat16() for f in feats], metas, d_region=float(g["d_region"]))
    with pytest.raises(RuntimeError, match="float32 features only"):
        (out.float() * gout).sum().backward()


# ------------------------------------------------------------------------------------------------------ the closed form
def _case(seed, Q, G, Tn, NP, D, N, hws, outside=False, three_cam=False):
    rng = np.random.default_rng(seed)
    P, L = NP * D, len(hws)
    qb = t(rng.random((1, Q, 10)))
    qb[..., 1] = 0.05 + 0.55 * qb[..., 1]
    if outside:
        qb[:, ::2, 1] = 1.3                                     # far outside the polar grid: clamped keypoints
    qb[..., 6:8] = qb[..., 6:8] * 2 - 1
    qb[..., 8:10] = qb[..., 8:10] * 4 - 2
    img = (64, 176)
    l2i = t(np.stack(syn.ring_lidar2img(Tn, N, img, three_cam_front=three_cam))[None])
    return dict(feats=[t(rng.standard_normal((Tn * G, N, h, w, 64))) for h, w in hws], query_bbox=qb,
                off=t(rng.uniform(-1.5, 1.5, (1, Q, G * P * 3))), ray=t(rng.standard_normal((1, Q, D))),
                sc=t(rng.standard_normal((1, Q, G * Tn * P * L))), td=t(rng.random((1, Tn)) + np.arange(Tn) * 0.5), l2i=l2i,
                T=Tn, G=G, NP=NP, D=D, pc=list(syn.PC_RANGE), d_region=0.1, image_h=img[0], image_w=img[1]), \
        t(rng.standard_normal((1, Q, G, Tn * P, 64)))


@pytest.mark.parametrize("shape", [(6, 4, 2, 2, 3, 2, [(4, 12), (2, 6), (1, 3), (1, 2)], True, False, False),
                                   (5, 3, 3, 1, 2, 3, [(5, 9), (3, 4)], False, True, False),      # odd G*T: quirk Q1 is not the identity
                                   (4, 1, 1, 1, 1, 6, [(6, 16)], False, False, False),            # P = 1, L = 1
                                   (5, 2, 2, 2, 2, 3, [(4, 12), (2, 6)], True, True, True)])      # imposed cameras
def test_closed_form_backward_is_the_autograd_of_the_chain(shape):
    """every output of rac_sampling4d_bwd's table, formula by formula, against float64 autograd of the restated forward (the box
    table a leaf), with points no camera sees (sampled in camera 0), points with homo <= eps and points on an active clamp"""
    Q, G, Tn, NP, D, N, hws, outside, three_cam, forced = shape
    c, gout = _case(Q + G + Tn + N, Q, G, Tn, NP, D, N, hws, outside, three_cam)
    view_in = None
    if forced:
        view_in = torch.from_numpy(np.random.default_rng(3).integers(0, N, (Tn * G, Q, NP * D))).to(torch.uint8)
    got = SR.closed_form_bwd(gout=gout, view_in=view_in, **c)
    ch = got["chain"]
    if not forced and N <= 3:
        assert bool((~ch["any_valid"]).any()) and bool((ch["homo"] <= 1e-5).any())
    if outside:
        assert bool(((ch["ux"] < 0) | (ch["ux"] > 1) | (ch["uy"] < 0) | (ch["uy"] > 1)).any())
    leaves = {k: c[k].clone().requires_grad_() for k in ("off", "ray", "sc")}
    feats = [f.clone().requires_grad_() for f in c["feats"]]
    table = T.box_table_torch(c["query_bbox"], c["pc"]).requires_grad_()
    out, cc = SR.core64(**{**c, **leaves, "feats": feats}, box_table=table, view_in=view_in)
    cc["u"].retain_grad(), cc["v"].retain_grad(), cc["wl"].retain_grad()
    (out * gout).sum().backward()
    want = dict(grad_offsets=leaves["off"].grad, grad_ray=leaves["ray"].grad, grad_scale=leaves["sc"].grad, grad_box=table.grad,
                grad_u=cc["u"].grad, grad_v=cc["v"].grad, grad_wl=cc["wl"].grad)
    for k, w_ in want.items():
        assert (got[k] - w_).abs().max().item() < 1e-10 * max(1.0, w_.abs().max().item()), k
    for a, b in zip(got["grad_feats"], feats):
        assert (a - b.grad).abs().max().item() < 1e-11 * max(1.0, b.grad.abs().max().item())
    assert all(float(got["grad_box"][..., i].abs().max()) > 0 for i in range(8))
    # the magnitude sums bound the values they scale
    mag = SR.closed_form_bwd(gout=gout, view_in=view_in, magnitude=True, **c)
    for k in ("grad_offsets", "grad_ray", "grad_scale", "grad_box"):
        assert bool((mag[k] >= got[k].abs() * (1 - 1e-9)).all()), k
    # the negative control's reference differs where a clamp is active
    if outside:
        wrong = SR.closed_form_bwd(gout=gout, view_in=view_in, wrong_term=True, **c)
        assert (wrong["grad_offsets"] - got["grad_offsets"]).abs().max().item() > 1e-6


def test_the_modules_torch_route_agrees_with_the_restatement(golden_dir):
    """the existing differentiable route (torch keypoint chain + sampling_4d) and core64 state the same function: compared in
    float64 at the golden's inputs through their outputs' dependence on the offsets"""
    g = load_golden(golden_dir)
    G, Tn, NP, D, N, L = (int(x) for x in g["shape"])
    m = module_from(g, dtype=torch.float64)
    qr, qf, feats, metas, gout = inputs_from(g, dtype=torch.float64)
    lin = (m.sampling_offset(qf), m.ray_points_offset(qf), m.scale_weights(qf))
    h, w = (int(x) for x in g["image_hw"])
    out, _ = SR.core64(feats, qr, *lin, metas[0]["time_diff"], metas[0]["lidar2img"], Tn, G, NP, D, m.pc_range, float(g["d_region"]), h, w)
    assert rel_err(out, g["out"]) < TOL_OUT
    (out * gout).sum().backward()
    assert rel_err(qf.grad, g["g:query_feat"]) < TOL_GRAD and rel_err(qr.grad, g["g:query_ray"]) < TOL_GRAD


# ------------------------------------------------------------------------------------------------------ argument checks
def _lib_or_fail():
    try:
        return _lib.lib()
    except RuntimeError as e:
        pytest.fail(str(e))


def test_sampling4d_bwd_argument_errors():
    lib = _lib_or_fail()
    d = ctypes.c_void_p(16)                     # never dereferenced: every failing call below fails its checks first
    pc = (ctypes.c_float * 6)(*syn.PC_RANGE)
    db = (ctypes.c_float * 3)(-0.1, 0.0, 0.1)

    def last():
        return lib.rac_last_error().decode()

    def bwd(L=4, B=1, Tn=8, N=6, G=4, Q=900, NP=4, D=3, C=64, dtype=_lib.RAC_F32, ld=(144, 3, 1536), gld=(144, 3, 1536), ptr=d,
            table=d, host=True, levels=True, glevels=True, hw_ok=True, loc=None, w=None):
        feats = (ctypes.c_void_p * 8)(*([16] * 8)) if levels else (ctypes.c_void_p * 8)()
        gfeats = (ctypes.c_void_p * 8)(*([16] * 8)) if glevels else (ctypes.c_void_p * 8)()
        hw = (ctypes.c_int32 * 16)(*([4, 4] * 8 if hw_ok else [4, 0] * 8))
        return lib.rac_sampling4d_bwd(feats if ptr else None, hw, L, ptr, table, ptr, ptr, ptr, ptr, ptr, None, ptr, gfeats, ptr, ptr, ptr,
                                      ptr, None, None, loc, w, *ld, *gld, B, Tn, N, G, Q, NP, D, C, pc if host else None,
                                      db if host else None, 0.1, 256.0, 704.0, 1e-5, dtype, None)

    assert bwd(L=3) == -1 and "L=3" in last() and "rac_sampling4d_bwd" in last()
    assert bwd(C=32) == -1 and "C=32" in last()
    assert bwd(D=17) == -1 and "bad sizes" in last()
    assert bwd(Tn=0) == -1 and "bad sizes" in last()
    assert bwd(N=17) == -1 and "bad sizes" in last()
    assert bwd(NP=43) == -1 and "num_point exceed limits" in last()          # 43 * 3 points
    assert bwd(dtype=_lib.RAC_BF16) == -1 and "dtype 1" in last() and "float32 features only" in last()
    assert bwd(ld=(143, 3, 1536)) == -1 and "row strides" in last()
    assert bwd(ld=(144, 3, 1535)) == -1 and "row strides" in last()
    assert bwd(gld=(144, 2, 1536)) == -1 and "gradient row strides" in last()
    assert bwd(gld=(144, 3, 1535)) == -1 and "gradient row strides" in last()
    assert bwd(Tn=32, ld=(144, 3, 6144), gld=(144, 3, 6144)) == -1 and "LDS staging" in last()      # 1536 keypoints x 13 floats
    assert bwd(table=None) == -1 and "box_table is null" in last()
    assert bwd(ptr=None) == -1 and "null pointer" in last()
    assert bwd(host=False) == -1 and "null pointer" in last()
    assert bwd(loc=d) == -1 and "go together" in last()
    assert bwd(levels=False) == -1 and "level 0" in last()
    assert bwd(glevels=False) == -1 and "level 0" in last()
    assert bwd(hw_ok=False) == -1 and "level 0" in last()
    assert bwd(Q=0, ptr=None, table=None) == 0 and bwd(B=0, ptr=None, table=None) == 0     # empty: nothing to check or launch
