"""rac_bev_sampling_bwd on the MI355X.

1. Gather half: grad_value and the kernel's per-keypoint debug outputs (grad_loc_out, grad_attn_out) element by element against
   the float64 closed form of the MSDA backward evaluated at the forward's own loc_out, under the bound and the factors of
   tests/test_backward_f64_gpu.py (|got - ref| <= K * 2**-24 * A + TINY; K = 64 value, 16 attn, 16 loc), with that file's
   negative control (one tap dropped must fail every kind).
2. Chain tail: the four logit gradients and grad_box against the float64 Jacobian of the chain multiplied into the float64
   per-keypoint gradients of 1. (same linearisation point), same bound form, K = 64 (fixed-order sums of up to heads*T*P
   terms); A = the same sums with every term made non-negative.  The worst err / A per kind is printed and, for comparison,
   the same metric of torch's float32 autograd of forward_unfused on the GPU.
3. Module level against the reference's golden (B = 1 fused, B = 2 through forward_unfused).
4. f8 shape, both temp_radar settings: every module gradient against forward_unfused in float64.
5. Two runs: everything but grad_value bit-identical, grad_value within 1e-5 of its largest element.
6. The grad-mode output of the module equals its no_grad output bit for bit.

Measured on the MI355X (worst err / A in units of 2**-24; recorded in profiles/bev_sampling_bwd_f8.json): value 8.2 (K = 64), loc 1.0,
attn 1.0 (K = 16); offsets 9.0, ray 1.8, scale 0.6, queue 0.3, box 10.5 (K = 64) -- torch's float32 autograd of the unfused chain:
offsets 23.7, ray 4.7, scale 49.7, queue 8.9, box 6.9.
"""
import json
import os

import numpy as np
import pytest
import torch

import bev_sampling_ref as BR
from racformer_amd import synthetic as syn
from racformer_amd import transformer as T
from racformer_amd.fused import bev_sampling_backward, bev_sampling_fused, box_prep
from test_bev_sampling_grad_cpu import check_against_golden, inputs_from, load_golden, module_from

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
K = {"value": 64.0, "attn": 16.0, "loc": 16.0, "offsets": 64.0, "ray": 64.0, "scale": 64.0, "queue": 64.0, "box": 64.0}
TINY = 1e-30
WORST, YARD = {}, {}
PC = list(syn.PC_RANGE)


@pytest.fixture(scope="module", autouse=True)
def _report():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)
    print("\nworst err/A per gradient kind, in units of 2**-24 (bound K) -- kernel | torch float32 autograd of forward_unfused:")
    for k in sorted(WORST):
        print(f"  {k:>10s}: {WORST[k] / U:9.3f} (K = {K[k]:g}) | {YARD.get(k, float('nan')) / U:9.3f}")
    path = os.environ.get("RAC_BEV_BWD_ERR_LOG")        # where to keep the figures as JSON (the record under profiles/ is a copy)
    if path:
        with open(path, "w") as f:
            json.dump(dict(unit="2**-24", kernel={k: v / U for k, v in WORST.items()}, torch_f32_autograd={k: v / U for k, v in YARD.items()},
                           K=K), f, indent=1)


def _violations(kind, got, ref, A):
    got, ref, A = got.detach().cpu().double(), ref.detach().cpu().double(), A.detach().cpu().double()
    assert got.shape == ref.shape == A.shape, (got.shape, ref.shape, A.shape)
    err = (got - ref).abs()
    return err, ~(err <= K[kind] * U * A + TINY), A


def _worst(err, A):
    pos = (A > 0) & torch.isfinite(err)     # (non-finite: only the yardstick's autograd, at a keypoint on the map centre, r = 0)
    return float((err[pos] / A[pos]).max()) if bool(pos.any()) else 0.0


def check(name, kind, got, ref, A):
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite gradient written"
    err, bad, A64 = _violations(kind, got, ref, A)
    w = _worst(err, A64)
    WORST[kind] = max(WORST.get(kind, 0.0), w)
    print(f"  {name} {kind}: worst err/A = {w / U:.3f} x 2^-24")
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        pytest.fail(f"{name}: {int(bad.sum())} of {bad.numel()} {kind} elements outside {K[kind]:g}*2^-24*A (worst {w / U:.2f}); first at flat "
                    f"{i}: got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} A {float(A64.flatten()[i])!r}")


def must_fail(name, kind, got, wrong, A):
    _, bad, _ = _violations(kind, got, wrong, A)
    assert bool(bad.any()), f"negative control {name}: a reference with one tap dropped passed the {kind} check"


# ------------------------------------------------------------------------------------------------------------------ cases
def make_case(seed, Q, heads, Tn, NP, D, H, W, d_lo=0.05, d_hi=0.55, edges=False):
    """all keypoints inside the map (radius <= 0.6 * 65 m plus a few metres).
    ``edges``: offsets 0 and zero velocity for the first queries, their boxes on exact pixel centres / the map centre line"""
    rng = np.random.default_rng(seed)
    P = NP * D
    qb = rng.random((1, Q, 10), dtype=np.float32)
    qb[..., 1] = d_lo + (d_hi - d_lo) * qb[..., 1]
    qb[..., 6:8] = qb[..., 6:8] * 2 - 1
    qb[..., 8:10] = qb[..., 8:10] * 4 - 2
    off = rng.uniform(-1.5, 1.5, (1, Q, heads * P * 2)).astype(np.float32)
    if edges:
        qb[0, :2, 8:10] = 0
        qb[0, 0, 0:2] = (0.0, 0.0)          # radius 0: y = 0.5 exactly, an integer tap of a map with an odd H (h_im = H/2 - 0.5)
        qb[0, 1, 0:2] = (0.25, 0.3)
        off[0, :2] = 0
    c = dict(value=torch.from_numpy(rng.standard_normal((Tn, H * W, heads, 64), dtype=np.float32)), hw=(H, W),
             query_bbox=torch.from_numpy(qb), off=torch.from_numpy(off), ray=torch.from_numpy(rng.standard_normal((1, Q, D), dtype=np.float32)),
             sc=torch.from_numpy(rng.standard_normal((1, Q, heads * P), dtype=np.float32)),
             qu=torch.from_numpy(rng.standard_normal((1, Q, Tn), dtype=np.float32)),
             time_diff=torch.from_numpy((rng.random((1, Tn)) * 0.1 + np.arange(Tn) * 0.5).astype(np.float32)), T=Tn, heads=heads, NP=NP, D=D,
             pc=PC, d_region=0.1)
    return c, torch.from_numpy(rng.standard_normal((1, Q, heads * 64), dtype=np.float32))


def run_kernel(c, gout, debug=True):
    g = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}
    args = (g["value"], g["hw"], g["query_bbox"], g["off"], g["ray"], g["sc"], g["qu"], g["time_diff"])
    cfg = (g["T"], g["heads"], g["NP"], g["D"], PC, g["d_region"])
    table = box_prep(g["query_bbox"], PC)
    out, loc = bev_sampling_fused(*args, *cfg, debug=True, box_table=table)
    res = bev_sampling_backward(*args, gout.to(DEV), *cfg, box_table=table, debug=debug)
    torch.cuda.synchronize()
    names = ("value", "offsets", "ray", "scale", "queue", "box", "loc", "attn")
    return dict(zip(names, (r.cpu() for r in res))), loc.cpu(), table.cpu(), out.cpu()


def reference(c, gout, loc, table):
    kw = dict(gout=gout, box_table=table, f32_coords=True, loc_at=loc, **c)
    return BR.closed_form_bwd(**kw), BR.closed_form_bwd(magnitude=True, **kw)


def drop_one_tap(c, gout, loc, ref):
    """the gather-half references with the heaviest tap of one keypoint missing"""
    H, W = c["hw"]
    Q, heads, Tn, P = loc.shape[1:5]
    qw = torch.softmax(c["qu"].double()[0], -1)
    aw = torch.softmax(c["sc"].double()[0].reshape(Q, heads, P), -1)
    taps = BR._taps(loc.double()[0], H, W, True)
    idx, tw, dh, dw, ok = taps[0]
    cand = ok.flatten().nonzero().flatten()[:64]
    k = int(cand[torch.argmax(tw.flatten()[cand])])
    q, h, t_, p = np.unravel_index(k, (Q, heads, Tn, P))
    g = gout.double().reshape(Q, heads, 64)[q, h]
    key = int(idx[q, h, t_, p])
    v = c["value"].double()[t_, key, h]
    at = float(aw[q, h, p] * qw[q, t_])
    dot = float((g * v).sum())
    wrong = {k_: ref["grad_" + k_].clone() for k_ in ("value", "loc", "attn")}
    wrong["value"][t_, key, h] -= float(tw[q, h, t_, p]) * at * g
    wrong["attn"][0, q, h, t_, p] -= float(tw[q, h, t_, p]) * dot
    wrong["loc"][0, q, h, t_, p, 0] -= W * at * float(dw[q, h, t_, p]) * dot
    wrong["loc"][0, q, h, t_, p, 1] -= H * at * float(dh[q, h, t_, p]) * dot
    return wrong


def yardstick(c, gout):
    """torch's float32 autograd of the module's unfused chain on the GPU (what existed before the fused backward): the four logit
    gradients and the gradient of the box table -> same kinds as the kernel's"""
    heads, Tn, NP, D = c["heads"], c["T"], c["NP"], c["D"]
    H, W = c["hw"]
    Q = c["query_bbox"].shape[1]
    m = T.BEVSampling(embed_dims=heads * 64, num_frames=Tn, num_points=NP, num_heads=heads, num_levels=1, pc_range=PC,
                      spatial_shapes=(W, H), depth_num=D).to(DEV)
    m.attention.num_heads = heads
    lv = {k: c[k].to(DEV).requires_grad_() for k in ("off", "ray", "sc", "qu")}
    table = box_prep(c["query_bbox"].to(DEV), PC).requires_grad_()
    # the chain from the box table on, in float32 torch ops (keypoints() starts at query_ray; its table is this one)
    loc = BR.chain64(table[0], c["query_bbox"].to(DEV)[0, :, 8:10], lv["off"][0], lv["ray"][0], c["time_diff"].to(DEV)[0], heads, NP, D, PC,
                     c["d_region"], dtype=torch.float32)[None]
    sw = torch.softmax(lv["sc"].reshape(1, Q, heads, 1, 1, NP * D), -1).expand(1, Q, heads, Tn, 1, NP * D).contiguous()
    aw = sw.view(1, Q, heads, Tn, 1, NP * D).permute(3, 0, 1, 2, 4, 5).reshape(Tn, Q, heads, 1, NP * D).contiguous()
    lo = loc.view(1, Q, heads, Tn, 1, NP * D, 2).permute(3, 0, 1, 2, 4, 5, 6).reshape(Tn, Q, heads, 1, NP * D, 2).contiguous()
    o = T._BEVAttendGather.apply(c["value"].to(DEV), lo, aw, [list(c["hw"])])              # [T,Q,C]
    out = (o * torch.softmax(lv["qu"], -1)[0].t()[:, :, None]).sum(0)[None]
    (out * gout.to(DEV)).sum().backward()
    return dict(offsets=lv["off"].grad.cpu(), ray=lv["ray"].grad.cpu(), scale=lv["sc"].grad.cpu(), queue=lv["qu"].grad.cpu(),
                box=table.grad.cpu())


CASES = {
    "h4 P10 T3 12x10": (1, 9, 4, 3, 2, 5, 12, 10),
    "h4 P20 T8 128x128": (2, 12, 4, 8, 4, 5, 128, 128),
    "h1 P7 T1 16x16": (3, 6, 1, 1, 7, 1, 16, 16),          # ragged P (not a multiple of 4), one frame, one head
    "h3 P9 T8 8x16": (4, 7, 3, 8, 3, 3, 8, 16),            # three heads
    "h4 P6 T2 15x15 edges": (5, 5, 4, 2, 2, 3, 15, 15),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_float64(name):
    c, gout = make_case(*CASES[name], edges="edges" in name)
    got, loc, table, _ = run_kernel(c, gout)
    ref, mag = reference(c, gout, loc, table)
    for kind in ("value", "loc", "attn"):
        check(name, kind, got[kind].reshape(ref["grad_" + kind].shape), ref["grad_" + kind], mag["grad_" + kind])
    wrong = drop_one_tap(c, gout, loc, ref)
    for kind in ("value", "loc", "attn"):
        must_fail(name, kind, got[kind].reshape(wrong[kind].shape), wrong[kind], mag["grad_" + kind])
    yard = yardstick(c, gout)
    for kind, key in (("offsets", "grad_offsets"), ("ray", "grad_ray"), ("scale", "grad_scale"), ("queue", "grad_queue"), ("box", "grad_box")):
        err, _, A = _violations(kind, yard[kind], ref[key], mag[key])
        YARD[kind] = max(YARD.get(kind, 0.0), _worst(err, A))
        check(name, kind, got[kind], ref[key], mag[key])
    assert float(got["box"][..., [2, 5]].abs().max()) == 0.0


def test_keypoints_beyond_the_map():
    """a whole case clearly outside: a velocity of 100 .. 150 m/s per axis over time differences >= 1 s carries every keypoint at
    least 39 m beyond the map in both coordinates.  Both are clamped: the chain gets no gradient at all (offsets, ray logits and
    box exactly 0), while the corner pixel the clamped location taps still feeds the value and the two softmaxes"""
    c, gout = make_case(6, 8, 4, 3, 2, 5, 16, 16)
    rng = np.random.default_rng(60)
    c["query_bbox"][0, :, 8:10] = torch.from_numpy((rng.uniform(100, 150, (8, 2)) * rng.choice([-1.0, 1.0], (8, 2))).astype(np.float32))
    c["time_diff"] = c["time_diff"] + 1.0
    got, loc, table, _ = run_kernel(c, gout)
    assert bool(((loc == 0) | (loc == 1)).all())
    ref, mag = reference(c, gout, loc, table)
    for kind, key in (("value", "grad_value"), ("offsets", "grad_offsets"), ("ray", "grad_ray"), ("scale", "grad_scale"),
                      ("queue", "grad_queue"), ("box", "grad_box"), ("loc", "grad_loc"), ("attn", "grad_attn")):
        check("beyond", kind, got[kind].reshape(ref[key].shape), ref[key], mag[key])
    for kind in ("offsets", "ray", "box"):
        assert float(got[kind].abs().max()) == 0.0, kind
    assert float(got["scale"].abs().max()) > 0 and float(got["value"].abs().max()) > 0


def test_non_finite_rows_stay_in_their_rows():
    c, gout = make_case(7, 6, 4, 3, 2, 5, 16, 16)
    c["query_bbox"][0, 1, 0] = float("nan")
    c["sc"][0, 2, 3] = float("inf")
    c["off"][0, 3, 5] = float("nan")
    got, _, _, _ = run_kernel(c, gout)
    keep = [0, 4, 5]
    for kind in ("offsets", "ray", "scale", "queue", "box", "loc", "attn"):
        assert bool(torch.isfinite(got[kind][0, keep]).all()), kind
    c2, _ = make_case(7, 6, 4, 3, 2, 5, 16, 16)
    got2, _, _, _ = run_kernel(c2, gout)
    for kind in ("offsets", "ray", "scale", "queue", "box"):
        assert torch.equal(got[kind][0, keep], got2[kind][0, keep]), kind


def test_two_runs_are_reproducible():
    c, gout = make_case(8, 900, 4, 8, 4, 5, 128, 128)
    a, _, _, _ = run_kernel(c, gout)
    b, _, _, _ = run_kernel(c, gout)
    for kind in ("offsets", "ray", "scale", "queue", "box", "loc", "attn"):
        assert torch.equal(a[kind], b[kind]), kind
    assert (a["value"] - b["value"]).abs().max().item() <= 1e-5 * a["value"].abs().max().item()


# ------------------------------------------------------------------------------------------------------------ module level
def _golden_on_gpu(g, pre):
    qr, qf, bev, metas, gout = inputs_from(g, pre)
    qr, qf, bev = (x.detach().to(DEV).requires_grad_() for x in (qr, qf, bev))
    return qr, qf, bev, [dict(time_diff=metas[0]["time_diff"].to(DEV))], gout.to(DEV)


@pytest.mark.parametrize("pre", ["b1:", "b2:"])
def test_module_against_the_reference_golden(golden_dir, pre):
    """B = 1 through the fused kernels, B = 2 through forward_unfused (rac_msda_fwd / rac_msda_bwd)"""
    g = load_golden(golden_dir)
    m = module_from(g).to(DEV)
    qr, qf, bev, metas, gout = _golden_on_gpu(g, pre)
    from racformer_amd import _lib
    _lib.timer = _lib.KernelTimer(only={"bev_sampling_fwd", "bev_sampling_bwd"})
    try:
        out = m(qr, qf, bev, metas, d_region=float(g["d_region"]))
        (out * gout).sum().backward()
        torch.cuda.synchronize()
        launches = {k: len(v) for k, v in _lib.timer.events.items()}
    finally:
        _lib.timer = None
    assert launches == (dict(bev_sampling_fwd=1, bev_sampling_bwd=1) if pre == "b1:" else {})
    check_against_golden(g, pre, m, qr, qf, bev, out)


@pytest.mark.parametrize("temp_radar", [False, True])
def test_f8_module_gradients_against_the_unfused_float64_path(temp_radar):
    """B = 1, Q = 900, T = 8, 4 heads, P = 20, 128 x 128: every module gradient against forward_unfused in float64 (CPU, the MSDA
    operator restated by the oracle)"""
    from test_bev_sampling_grad_cpu import fake_msda_bwd, fake_msda_fwd
    torch.manual_seed(5)
    kw = dict(embed_dims=256, num_frames=8, num_points=4, num_heads=4, num_levels=1, pc_range=PC, spatial_shapes=(128, 128), depth_num=5,
              temp_radar=temp_radar)
    m = T.BEVSampling(**kw).eval()
    with torch.no_grad():
        torch.nn.init.normal_(m.sampling_offset.weight, std=0.02)
        torch.nn.init.normal_(m.attention.value_proj.bias, std=0.1)
    m64 = T.BEVSampling(**kw).eval().double()                     # the float64 reference on the CPU
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
    rng = np.random.default_rng(9)
    qr = rng.random((1, 900, 10), dtype=np.float32)
    qr[..., 1] = 0.05 + 0.55 * qr[..., 1]
    qr[..., 6:8] = qr[..., 6:8] * 2 - 1
    qr[..., 8:10] = qr[..., 8:10] * 4 - 2
    qf = rng.standard_normal((1, 900, 256), dtype=np.float32)
    C_in = 256
    bev = (rng.standard_normal((1, 8, C_in, 128, 128), dtype=np.float32) * np.float32(0.5))
    td = (np.arange(8, dtype=np.float32) * np.float32(0.5))[None]
    gout = rng.standard_normal((1, 900, 256), dtype=np.float32)
    # Keypoints within reach of the float32 / float64 difference of a location (a few 1e-7 of the map) of a pixel-cell border pick
    # different taps in the two evaluations, and the gradient of a bilinear sample jumps there: keep all 576,000 of them 1e-5 of the
    # map away (the case stays inside the map: no clamp).
    td64 = torch.from_numpy(td).double()
    qf64 = BR.nudge_query_feat(m64, torch.from_numpy(qr).double(), torch.from_numpy(qf).double(), td64, (128, 128), 0.1, 1e-5)
    qf = qf64.float().numpy()
    with torch.no_grad():
        x = torch.from_numpy(qf).double()
        dmin = float(BR.border_distance(torch.from_numpy(qr).double(), m64.sampling_offset(x), m64.ray_points_offset(x), td64, 4, 4, 5, 128,
                                        128, PC, 0.1).min())
    assert dmin >= 1e-5, dmin
    i64 = [torch.from_numpy(a).double().requires_grad_() for a in (qr, qf, bev)]
    saved = T.msda_forward, T.msda_backward
    T.msda_forward, T.msda_backward = fake_msda_fwd, fake_msda_bwd
    try:
        value, hw = m64.prepare_value(i64[2])
        want = m64.forward_unfused(i64[0], i64[1], value, hw, torch.from_numpy(td).double(), 0.1)
        (want * torch.from_numpy(gout).double()).sum().backward()
    finally:
        T.msda_forward, T.msda_backward = saved
    mg = m.to(DEV)
    ig = [torch.from_numpy(a).to(DEV).requires_grad_() for a in (qr, qf, bev)]
    out = mg(ig[0], ig[1], ig[2], [dict(time_diff=torch.from_numpy(td).to(DEV))], d_region=0.1)
    (out * torch.from_numpy(gout).to(DEV)).sum().backward()
    torch.cuda.synchronize()

    def rel(a, b):
        return ((a.detach().cpu().double() - b.detach()).abs().max() / b.detach().abs().max()).item()

    worst = {"out": rel(out, want)}
    worst.update({n: rel(a.grad, b.grad) for n, a, b in (("query_ray", ig[0], i64[0]), ("query_feat", ig[1], i64[1]), ("bev_feats", ig[2], i64[2]))})
    p64 = dict(m64.named_parameters())
    for n, p in mg.named_parameters():
        assert p.grad is not None, n
        worst[n] = rel(p.grad, p64[n].grad)
    print("\n" + "\n".join(f"  {k:>44s}: {v:.2e}" for k, v in worst.items()))
    # Tolerance (max |err| / max |value| per tensor) from the float32 layers around the kernel, fixed before any figure was seen:
    # a float32 sum of K terms rounds about sqrt(K) * 2**-24 of its magnitude, the largest of ~1e5 .. 1e7 elements about 5 times
    # that, and L layers in sequence add in quadrature: 5 * sqrt(K) * 2**-24 * sqrt(L).
    #   rows (out, query_feat, query_ray): the 640-tap gather and a 256-term GEMM, K = 896; L = 3 (value_proj, gather, output_proj /
    #   the Linears)                                                                         -> 1.5e-5
    #   reduced tensors (parameters, bev_feats): sums over up to all 8 x 16384 pixels (value_proj.weight), K = 131072, L = 3 -> 1.9e-4
    #   radar stream: the ConvGRU over 8 frames (three convolutions a step), down / upsampling, fusion and value_proj in front of
    #   the same, L = 30: both times sqrt(10)                                                   -> 4.9e-5, 5.9e-4
    f = 10 ** 0.5 if temp_radar else 1.0
    tol_rows = 5 * 896 ** 0.5 * U * 3 ** 0.5 * f
    tol_reduced = 5 * 131072 ** 0.5 * U * 3 ** 0.5 * f
    bad = {k: v for k, v in worst.items() if not v < (tol_rows if k in ("out", "query_feat", "query_ray") else tol_reduced)}
    assert not bad, bad


@pytest.mark.parametrize("with_boxes", [False, True])
def test_grad_mode_output_is_the_no_grad_output(golden_dir, with_boxes):
    g = load_golden(golden_dir)
    m = module_from(g).to(DEV)
    qr, qf, bev, metas, _ = inputs_from(g, "b1:")
    qr, qf, bev = qr.detach().to(DEV).requires_grad_(with_boxes), qf.detach().to(DEV), bev.detach().to(DEV)
    metas = [dict(time_diff=metas[0]["time_diff"].to(DEV))]
    with torch.no_grad():
        a = m(qr, qf, bev, metas, d_region=0.1)
    b = m(qr, qf, bev, metas, d_region=0.1)
    assert b.grad_fn is not None and a.grad_fn is None
    assert torch.equal(a, b.detach())
