"""rac_bev_sampling_bwd_batch on the MI355X: the BEV sampling backward for B > 1, with the reference's frame / batch pairing.

1. Kernel level: every output element by element against the float64 closed form of tests/bev_sampling_batch_ref.py evaluated at
   the forward's own loc_out, under the bound and the factors of tests/test_bev_sampling_grad_gpu.py (|got - ref| <= K * 2**-24 * A
   + TINY; its K, check, must_fail).  (B, T) in {(2, 3), (3, 4), (2, 2), (4, 2)}: B not dividing T, B dividing T, B > T; heads 4 and
   1; (NP, D) = (2, 5) and (1, 3); maps 12 x 10 and 8 x 8; one case with queries beyond the map (clamped keypoints).  Two cases of
   this file's own: a 128 x 128 map, where one ulp of a location is 8e-6 of a tap weight -- a backward whose keypoints were not
   the forward's bits would show --, and B = 4 at T = 8, heads 4, P = 20, whose workgroup stages 77 KB of LDS (above the 64 KB a
   launch may ask for without raising the kernel's limit).
2. Negative controls: one tap dropped must fail value / loc / attn; a reference with the pairing undone (the locations and point
   weights of (b_o, t_o) for row r) must fail every gradient kind at (B, T) = (2, 3) -- after checking on the CPU that the two
   pairings differ by far more than the bound on that input.
3. B = 1 through the new symbol against rac_bev_sampling_bwd: every output but grad_value bit-identical, grad_value within 1e-5 of
   its largest element.  Both symbols against a pin of the build before the two kernels became two instantiations of one source
   (tests/golden/bev_bwd_pin.npz): every output but grad_value bit for bit, on the smallest cases that enter every loop's second trip.
4. Two runs at B = 2, f8 shape (Q = 900, T = 8, heads 4, P = 20, 128 x 128): the same criterion.
5. Module level: the ``b2:`` golden of the reference through attend_prepared(..., fused_batch=True): one forward and one backward
   launch of the fused kernels; the grad-mode output is the no_grad output bit for bit.
6. Decoder level: the rig of tests/decoder_grad_ref.py at B = 2: forward_train launches bev_sampling_bwd twice per layer call and
   rac_msda_bwd never (counted at transformer.msda_backward); every parameter and input gradient agrees with the same layer with
   the fused batch route switched off.

Measured on the MI355X (worst err / A in units of 2**-24; recorded in profiles/bev_sampling_bwd_batch_f8.json): value 8.8 (K = 64), loc 1.1,
attn 1.0 (K = 16); offsets 1.8, ray 4.6, scale 0.6, queue 0.5, box 0.5 (K = 64).  Decoder level: the fused route's closest tensor to its bound
6.3e-6 of 1e-5 (sampling_lss_bev.ray_points_offset.bias; the unfused route's: 6.4e-6); the two routes at most 6.1e-6 apart where 2e-5 is allowed."""
import json
import os

import numpy as np
import pytest
import torch

import bev_sampling_batch_ref as BB
import bev_sampling_ref as BR
import decoder_grad_ref as DR
import test_bev_sampling_grad_gpu as G
from racformer_amd import _lib
from racformer_amd import synthetic as syn
from racformer_amd import transformer as T
from golden import gen_bev_bwd_pin as pin
from racformer_amd.fused import bev_sampling_backward, bev_sampling_fused, box_prep
from test_bev_sampling_batch_grad_cpu import case
from test_bev_sampling_grad_cpu import check_against_golden, inputs_from, load_golden, module_from
from test_bev_sampling_grad_gpu import K, check, must_fail

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
PC = list(syn.PC_RANGE)
WORST = {}
NAMES = ("value", "offsets", "ray", "scale", "queue", "box", "loc", "attn")
KINDS = tuple((k, "grad_" + k) for k in NAMES)


@pytest.fixture(scope="module", autouse=True)
def _report():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield
    torch.set_num_threads(n)
    print("\nrac_bev_sampling_bwd_batch: worst err/A per gradient kind, in units of 2**-24 (bound K):")
    for k in sorted(WORST):
        print(f"  {k:>10s}: {WORST[k] / U:9.3f} (K = {K[k]:g})")
    path = os.environ.get("RAC_BEV_BWD_BATCH_ERR_LOG")
    if path:
        with open(path, "w") as f:
            json.dump(dict(unit="2**-24", kernel={k: v / U for k, v in WORST.items()}, K=K), f, indent=1)


def checked(name, kind, got, ref, A):
    err, _, A64 = G._violations(kind, got, ref, A)
    WORST[kind] = max(WORST.get(kind, 0.0), G._worst(err, A64))
    check(name, kind, got, ref, A)


def run_kernel(c, gout, batch_symbol=None):
    g = {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in c.items()}
    args = (g["value"], g["hw"], g["query_bbox"], g["off"], g["ray"], g["sc"], g["qu"], g["time_diff"])
    cfg = (g["T"], g["heads"], g["NP"], g["D"], PC, g["d_region"])
    table = box_prep(g["query_bbox"], PC)
    _, loc = bev_sampling_fused(*args, *cfg, debug=True, box_table=table)
    res = bev_sampling_backward(*args, gout.to(DEV), *cfg, box_table=table, debug=True, batch_symbol=batch_symbol)
    torch.cuda.synchronize()
    return dict(zip(NAMES, (r.cpu() for r in res))), loc.cpu(), table.cpu()


def reference(c, gout, loc, table, **kw):
    kw = dict(gout=gout, box_table=table, f32_coords=True, loc_at=loc, **c, **kw)
    return BB.closed_form_bwd_batch(**kw), BB.closed_form_bwd_batch(magnitude=True, **kw)


def drop_one_tap(c, gout, loc, ref):
    """the gather-half references with the heaviest tap of one keypoint of output sample 0 missing"""
    H, W = c["hw"]
    B, Q, heads, Tn, P = loc.shape[:5]
    b_l = BB.pairing(B, Tn)[2]
    qw = torch.softmax(c["qu"].double(), -1)
    aw = torch.softmax(c["sc"].double().reshape(B, Q, heads, P), -1)
    idx, tw, dh, dw, ok = BR._taps(loc.double()[0], H, W, True)[0]             # [Q,heads,T,P] of output sample 0: rows 0 .. T-1
    cand = ok.flatten().nonzero().flatten()[:64]
    k = int(cand[torch.argmax(tw.flatten()[cand])])
    q, h, t_, p = np.unravel_index(k, (Q, heads, Tn, P))
    g = gout.double().reshape(B, Q, heads, 64)[0, q, h]
    key = int(idx[q, h, t_, p])
    v = c["value"].double()[t_, key, h]
    at = float(aw[int(b_l[t_]), q, h, p] * qw[0, q, t_])
    dot = float((g * v).sum())
    wrong = {k_: ref["grad_" + k_].clone() for k_ in ("value", "loc", "attn")}
    wrong["value"][t_, key, h] -= float(tw[q, h, t_, p]) * at * g
    wrong["attn"][0, q, h, t_, p] -= float(tw[q, h, t_, p]) * dot
    wrong["loc"][0, q, h, t_, p, 0] -= W * at * float(dw[q, h, t_, p]) * dot
    wrong["loc"][0, q, h, t_, p, 1] -= H * at * float(dh[q, h, t_, p]) * dot
    return wrong


# name -> (seed, B, T, Q, heads, NP, D, H, W, queries beyond the map)
CASES = {
    "B2 T3 h4 P10 12x10": (21, 2, 3, 6, 4, 2, 5, 12, 10, False),
    "B3 T4 h1 P3 8x8": (22, 3, 4, 6, 1, 1, 3, 8, 8, False),
    "B2 T2 h4 P3 8x8": (23, 2, 2, 6, 4, 1, 3, 8, 8, False),
    "B4 T2 h1 P10 12x10 beyond": (24, 4, 2, 6, 1, 2, 5, 12, 10, True),
    "B2 T3 h4 P20 128x128": (25, 2, 3, 6, 4, 4, 5, 128, 128, False),
    "B4 T8 h4 P20 16x16 77KB": (26, 4, 8, 6, 4, 4, 5, 16, 16, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_against_float64(name):
    *dims, beyond = CASES[name]
    # Eight frames carry a keypoint up to 7 m (2 m/s over 3.6 s) beside its offsets' 4 m: a query nearer than that to the map centre
    # has keypoints passing it, where sqrt and atan2 of (ex, ey) -- each rounded to 3e-6 m in float32 -- are ill-conditioned (relative
    # 3e-6 m / r: 2e-4 at r = 1.5 cm), which a bound in units of 2**-24 of the magnitudes does not model.  That case keeps its
    # queries 19.5 m out; the others (T <= 4, within 1.7 s) draw theirs as tests/test_bev_sampling_grad_gpu.py does.
    c, gout = case(*dims, outside=beyond, dtype=np.float32, d_lo=0.3 if dims[2] == 8 else 0.05)
    got, loc, table = run_kernel(c, gout)
    if beyond:
        assert bool(((loc == 0) | (loc == 1)).any())
    ref, mag = reference(c, gout, loc, table)
    for kind, key in KINDS:
        checked(name, kind, got[kind].reshape(ref[key].shape), ref[key], mag[key])
    wrong = drop_one_tap(c, gout, loc, ref)
    for kind in ("value", "loc", "attn"):
        must_fail(name, kind, got[kind].reshape(wrong[kind].shape), wrong[kind], mag["grad_" + kind])
    assert float(got["box"][..., [2, 5]].abs().max()) == 0.0


def test_a_reference_with_the_pairing_undone_fails_every_kind():
    """(B, T) = (2, 3): rows 1 .. 4 of 6 are paired with another (sample, frame) than their own"""
    *dims, _ = CASES["B2 T3 h4 P10 12x10"]
    c, gout = case(*dims, dtype=np.float32)
    # on the CPU first: the two pairings, both at their float64 chain's locations, differ by far more than the bound in every kind
    paired, mag = BB.closed_form_bwd_batch(gout=gout, **c), BB.closed_form_bwd_batch(gout=gout, magnitude=True, **c)
    undone = BB.closed_form_bwd_batch(gout=gout, paired=False, **c)
    for kind, key in KINDS:
        far = (paired[key] - undone[key]).abs() > 1000 * K[kind] * U * mag[key]
        assert int(far.sum()) >= 0.1 * far.numel(), (kind, int(far.sum()), far.numel())
    got, loc, table = run_kernel(c, gout)
    ref, mag = reference(c, gout, loc, table)
    for kind, key in KINDS:
        check("pairing", kind, got[kind].reshape(ref[key].shape), ref[key], mag[key])
        must_fail("pairing undone", kind, got[kind].reshape(undone[key].shape), undone[key], mag[key])


def _same_but_value(a, b):
    for kind in NAMES[1:]:
        assert torch.equal(a[kind], b[kind]), kind
    assert (a["value"] - b["value"]).abs().max().item() <= 1e-5 * a["value"].abs().max().item()


@pytest.mark.parametrize("dims", [(31, 1, 3, 9, 4, 2, 5, 12, 10), (32, 1, 8, 12, 4, 4, 5, 128, 128), (33, 1, 1, 6, 1, 7, 1, 16, 16)])
def test_b1_through_the_new_symbol_is_the_old_kernel(dims):
    c, gout = case(*dims, dtype=np.float32)
    old, _, _ = run_kernel(c, gout, batch_symbol=False)
    new, _, _ = run_kernel(c, gout, batch_symbol=True)
    _same_but_value(old, new)


def test_two_runs_are_reproducible_b2_f8():
    c, gout = case(34, 2, 8, 900, 4, 4, 5, 128, 128, dtype=np.float32)
    a, _, _ = run_kernel(c, gout)
    b, _, _ = run_kernel(c, gout)
    _same_but_value(a, b)
    assert float(a["offsets"].abs().max()) > 0 and bool(torch.isfinite(a["value"]).all())


@pytest.mark.parametrize("name,batch_symbol", [(n, b) for n in pin.CASES for b in pin.symbols(n)])
def test_single_writer_outputs_are_the_pinned_ones(golden_dir, name, batch_symbol):
    """every output but grad_value, bit for bit as the build of the commit before the two kernels became one source returned it on the
    MI355X (tests/golden/gen_bev_bwd_pin.py, bev_bwd_pin.npz), through both symbols at B = 1"""
    with np.load(os.path.join(golden_dir, "bev_bwd_pin.npz")) as z:
        d = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "|")}
    assert tuple(d["case"]) == tuple(float(x) for x in pin.CASES[name])
    c, gout = pin.draw(name)
    # (float64 sums of up to 3e7 float32 values: their order, so their last bits, is the library's; another draw is off by O(1))
    assert np.allclose(pin.checksums(c, gout), d["checksums"], rtol=0, atol=1e-6), "the drawn inputs are not the pinned run's"
    got, loc, _ = run_kernel(c, gout, batch_symbol=batch_symbol)
    if pin.CASES[name][9]:
        assert bool(((loc == 0) | (loc == 1)).any())
    for kind in pin.OUTPUTS:
        want = torch.from_numpy(d["grad_" + kind])
        assert torch.equal(got[kind].reshape(want.shape), want), (name, batch_symbol, kind)


# ------------------------------------------------------------------------------------------------------------ module level
def _golden_on_gpu(g, pre):
    qr, qf, bev, metas, gout = inputs_from(g, pre)
    qr, qf, bev = (x.detach().to(DEV).requires_grad_() for x in (qr, qf, bev))
    return qr, qf, bev, metas[0]["time_diff"].to(DEV), gout.to(DEV)


def test_module_fused_batch_against_the_reference_golden(golden_dir):
    g = load_golden(golden_dir)
    m = module_from(g).to(DEV)
    qr, qf, bev, td, gout = _golden_on_gpu(g, "b2:")
    _lib.timer = _lib.KernelTimer(only={"bev_sampling_fwd", "bev_sampling_bwd"})
    try:
        value, hw = m.prepare_value(bev)
        out = m.attend_prepared(qr, qf, value, hw, td, float(g["d_region"]), fused_batch=True)
        (out * gout).sum().backward()
        torch.cuda.synchronize()
        launches = {k: len(v) for k, v in _lib.timer.events.items()}
    finally:
        _lib.timer = None
    assert launches == dict(bev_sampling_fwd=1, bev_sampling_bwd=1)
    check_against_golden(g, "b2:", m, qr, qf, bev, out)


def test_module_grad_mode_output_is_the_no_grad_output_b2(golden_dir):
    g = load_golden(golden_dir)
    m = module_from(g).to(DEV)
    qr, qf, bev, td, _ = _golden_on_gpu(g, "b2:")
    with torch.no_grad():
        value, hw = m.prepare_value(bev)
        a = m.attend_prepared(qr, qf, value, hw, td, 0.1, fused_batch=True)
    b = m.attend_prepared(qr, qf, value, hw, td, 0.1, fused_batch=True)
    assert b.grad_fn is not None and a.grad_fn is None
    assert torch.equal(a, b.detach())


# ----------------------------------------------------------------------------------------------------------- decoder level
def _draw_b2(seeds):
    ds = [DR.draw(int(s)) for s in seeds]
    return {k: np.concatenate([d[k] for d in ds], axis=0) for k in ds[0]}


def _run_layer_b2(layer, d):
    """DR.run_layer on a drawn batch, with the launches of the BEV kernels counted"""
    t = lambda k: torch.from_numpy(np.asarray(d[k]).astype(np.float32)).to(DEV)  # noqa: E731
    leaves = {k: t(k).requires_grad_() for k in ("query_bbox", "query_feat", "lss", "radar")}
    leaves.update({f"feat{i}": t(f"feat{i}").requires_grad_() for i in range(len(DR.HWS))})
    td_safe = t("time_diff").clone()
    td_safe[td_safe < 1e-5] = 1.0
    metas = [dict(img_shape=[(DR.IMG_HW[0], DR.IMG_HW[1], 3)], time_diff=t("time_diff"), lidar2img=t("lidar2img"), time_diff_safe=td_safe)]
    layer.zero_grad(set_to_none=True)
    layer._carry = None
    _lib.timer = _lib.KernelTimer(only={"bev_sampling_fwd", "bev_sampling_bwd", "msda_fwd"})
    try:
        feat, cls, pred = layer(leaves["query_bbox"], leaves["query_feat"], [leaves[f"feat{i}"] for i in range(len(DR.HWS))], leaves["lss"],
                                leaves["radar"], None, metas, layer=DR.LAYER)
        xy = layer.last_bbox_xy
        ((feat * t("gout_feat")).sum() + (cls * t("gout_cls")).sum() + (xy * t("gout_xy")).sum()).backward()
        torch.cuda.synchronize()
        launches = {k: len(v) for k, v in _lib.timer.events.items()}
    finally:
        _lib.timer = None
    out = dict(out_feat=feat, out_cls=cls, out_pred=pred, out_xy=xy)
    return {k: v.detach().cpu().numpy() for k, v in out.items()}, DR.grads_of(layer, leaves), launches


def test_decoder_layer_trains_at_b2_on_the_fused_bev_kernels(golden_dir, monkeypatch):
    """One call of the layer under autograd at B = 2 on the inputs of tests/golden/decoder_grad_small_b2.npz
    (gen_golden_decoder_grad_b2.py: the reference's own layer at B = 2 in float32 and float64).
    1. The training route stays on the fused BEV kernels: two forward and two backward launches, rac_msda_* never.
    2. Against the reference by the rule of tests/decoder_grad_ref.py: per gradient tensor within max(2 x the reference's own
       float32-against-float64 figure, 1e-5) of the float64 gradient's largest element; the outputs within 1e-5.
    3. Against the same layer with the fused batch route switched off (forward_unfused: rac_msda_fwd / rac_msda_bwd): both routes are
       held to the same float64 gradients by 2., so they differ by at most twice that bound per tensor."""
    g1 = DR.load_golden(golden_dir)
    with np.load(os.path.join(golden_dir, "decoder_grad_small_b2.npz")) as z:
        g = {k: z[k] for k in z.files}
    assert int(g["weight_seed"]) == int(g1["weight_seed"])
    layer = DR.build_layer(g1, device=DEV)
    d = _draw_b2(g["seeds"])
    msda_bwd_calls, real_msda_bwd = [], T.msda_backward
    monkeypatch.setattr(T, "msda_backward", lambda *a, **kw: (msda_bwd_calls.append(1), real_msda_bwd(*a, **kw))[1])
    out, grads, launches = _run_layer_b2(layer, d)
    assert launches == dict(bev_sampling_fwd=2, bev_sampling_bwd=2) and msda_bwd_calls == [], (launches, msda_bwd_calls)
    report = []
    bad = DR.check_against_golden(g, out, grads, "fused batch route", report)
    print("\nfused batch route, closest to the bound:",
          ", ".join(f"{k} {e:.1e} (ref {r:.1e})" for k, e, r, _ in sorted(report, key=lambda r: -r[1] / r[3])[:8]))
    monkeypatch.setattr(T, "bev_backward_batch_fits", lambda *a: False)
    out0, grads0, launches0 = _run_layer_b2(layer, d)
    assert launches0 == dict(msda_fwd=2) and len(msda_bwd_calls) == 2, (launches0, msda_bwd_calls)
    report0 = []
    bad0 = DR.check_against_golden(g, out0, grads0, "unfused route", report0)
    print("unfused route, closest to the bound:",
          ", ".join(f"{k} {e:.1e} (ref {r:.1e})" for k, e, r, _ in sorted(report0, key=lambda r: -r[1] / r[3])[:8]))
    worst = {}
    for k, v in out.items():
        e = float(np.abs(v.astype(np.float64) - out0[k]).max() / np.abs(g["out64_" + k[4:]]).max())
        worst[k] = (e, 2e-5)
    for k, v in grads.items():
        e = float(np.abs(v.astype(np.float64) - grads0[k]).max() / float(g["max64:" + k]))
        worst[k] = (e, 2 * DR.bound(g["ref:" + k]))
    print("fused against unfused, closest to twice the bound:",
          ", ".join(f"{k} {e:.1e} ({b:.1e})" for k, (e, b) in sorted(worst.items(), key=lambda kv: -kv[1][0] / kv[1][1])[:8]))
    assert not bad, "\n".join(bad)
    assert not bad0, "the comparator itself misses the reference:\n" + "\n".join(bad0)
    apart = {k: v for k, v in worst.items() if not v[0] <= v[1]}
    assert not apart, apart
