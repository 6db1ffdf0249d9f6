"""AdaptiveMixing's two big Linears (parameter_generator 256 -> N, out_proj K -> 256) in split precision under autograd on the
MI355X: the packs with a device-side scale, the two data gradients on the forward kernels, rac_linear_wgrad, the autograd
Function and the training route that composes them (AdaptiveMixing.forward_train, the switch AdaptiveMixing.fused_linear_grad).

  * every product element by element against float64 under ``|got - ref| <= 8 * 2**-24 * A`` with
    ``A = sum |a_k||b_k| + 2**-14 (amax_a sum |b_k| + amax_b sum |a_k|)``: the second term is the absolute step of the operand
    images (rac_act_scale brings amax into [2^13, 2^14), the f16 subnormal step of lo is 2^-24).  The worst err / A per product is
    printed, with the library's fp32 GEMM on the same inputs as context (no criterion);
  * negative control: against a reference with one index of the reduction dropped (a row m of the weight gradients' sum, a row
    of the weight operand of the data gradients) every product must fail the bound;
  * module gradients against the reference's own autograd (tests/golden/mixing_grad_small.npz).  The fixture's query_dim is 4,
    the kernels' 256: the fixture is embedded exactly -- query, gout, the generator's weight columns and out_proj's weight rows
    and bias zero-padded to 256 --, which leaves every stored value what it was and gives exact zeros in the padding;
  * the decoder layer of tests/decoder_grad_ref.py with the switch on: within the fixture's per-tensor bound, and bitwise equal
    over two runs of two chained layer calls wherever nothing scatters; with the switch off bitwise the route of before."""
import os

import numpy as np
import pytest
import torch

import decoder_grad_ref as DR
from mixing_ref import min_margin
from racformer_amd import fused as Fz
from racformer_amd import transformer as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
KF = 8.0
MARGIN = 2.0 ** -16
WORST, LIBRARY = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nworst err/A per product in units of 2**-24 (bound 8) | the library's fp32 GEMM on the same inputs:")
    for name in sorted(WORST):
        print(f"  {name:>10s}: {WORST[name] / U:8.3f} | {LIBRARY.get(name, float('nan')) / U:8.3f}")


@pytest.fixture
def switch_on(monkeypatch):
    monkeypatch.setattr(T.AdaptiveMixing, "fused_linear_grad", True)


def t(a):
    return torch.from_numpy(np.asarray(a)).clone()


def padded(rows, width, pad, gen, scale=1.0):
    """float32 [rows, width] as a column slice of rows width + pad wide, the padding NaN"""
    buf = torch.full((rows, width + pad), float("nan"), device=DEV)
    v = buf[:, :width]
    v.copy_((torch.randn(rows, width, generator=gen) * scale).to(DEV))
    return buf, v


def bound_A(a, b, amax_a, amax_b):
    """a [I, R], b [R, J] float64 (R: the reduction) -> (a @ b, A)"""
    aa, ab = a.abs(), b.abs()
    A = aa @ ab + 2.0 ** -14 * (amax_a * ab.sum(0)[None, :] + amax_b * aa.sum(1)[:, None])
    return a @ b, A


def check(name, got, ref, A, lib=None):
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite values (an element was not written)"
    err = (got.double() - ref).abs()
    pos = A > 0
    w = float((err[pos] / A[pos]).max()) if bool(pos.any()) else 0.0
    WORST[name] = max(WORST.get(name, 0.0), w)
    if lib is not None and bool(pos.any()):
        LIBRARY[name] = max(LIBRARY.get(name, 0.0), float(((lib.double() - ref).abs()[pos] / A[pos]).max()))
    bad = ~(err <= KF * U * A)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        pytest.fail(f"{name}: {int(bad.sum())} of {bad.numel()} outside 8*2^-24*A (worst err/A {w / U:.2f} x 2^-24); first at flat {i}: "
                    f"got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} A {float(A.flatten()[i])!r}")


def fails(got, ref, A):
    return bool((~((got.double() - ref).abs() <= KF * U * A)).any())


# ------------------------------------------------------------------------------------------------ packs
@pytest.mark.parametrize("M,K,pad", [(1, 32, 0), (17, 256, 4), (33, 4608, 8)])
def test_activation_pack_round_trip(M, K, pad):
    gen = torch.Generator().manual_seed(M + K)
    buf, v = padded(M, K, pad, gen, scale=3.0)
    v[0, 0] = 1e-7            # far below the image's step
    amax = Fz.absmax_device(v.contiguous())
    img = torch.full((M + 1, K // 32, 64), float("nan"), device=DEV, dtype=torch.float16)
    Fz.linear_pack_act(v, amax, out=img[:M])
    torch.cuda.synchronize()
    assert bool(torch.isnan(img[M]).all()), "written past the last row"
    a = float(amax)
    assert a == float(v.abs().max())
    scale = 2.0 ** (14 - np.frexp(a)[1])
    assert 2.0 ** 13 <= a * scale < 2.0 ** 14
    back = (img[:M, :, :32].double() + img[:M, :, 32:].double()).reshape(M, K)
    want = v.double() * scale
    err = (back - want).abs()
    # hi + lo carries 22 significant bits; below that the f16 subnormal step of lo, 2^-24, is what remains
    assert bool((err <= torch.maximum(want.abs() * 2.0 ** -22, torch.full_like(want, 2.0 ** -24))).all()), float(err.max())


def test_activation_pack_of_zeros_is_zero():
    v = torch.zeros(5, 64, device=DEV)
    img = Fz.linear_pack_act(v, Fz.absmax_device(v))
    assert float(img.abs().max()) == 0.0


@pytest.mark.parametrize("N,K", [(256, 128), (384, 256), (4608, 256), (256, 4608)])
def test_transposed_weight_pack_is_the_pack_of_the_transpose(N, K):
    w = (torch.randn(N, K, generator=torch.Generator().manual_seed(N + K)) * 0.07).to(DEV)
    img, alpha = Fz.pack_linear_weight_t(w)
    want, want_alpha = Fz.pack_gemm_split_weight(w.t().contiguous())
    assert tuple(img.shape) == (K, N // 32, 64) and torch.equal(img, want)
    assert alpha == want_alpha * Fz.SPLIT_ACT_SCALE


# ------------------------------------------------------------------------------------------------ the four products
class Case:
    """One M and one wide size ``Wd`` for all four products: out_proj with K = Wd (g [M,256], Z [M,Wd], W_out [256,Wd]) and the
    generator with N = Wd (query [M,256], dP [M,Wd], W_gen [Wd,256]); every row operand a slice of padded rows."""

    def __init__(self, M, Wd, gscale=1.0):
        gen = torch.Generator().manual_seed(1000 * M + Wd)
        self.M, self.Wd = M, Wd
        _, self.g = padded(M, 256, 4, gen)
        _, self.z = padded(M, Wd, 8, gen)
        _, self.q = padded(M, 256, 12, gen)
        _, self.dp = padded(M, Wd, 4, gen)
        self.g *= gscale
        self.dp *= gscale
        self.w_out = (torch.randn(256, Wd, generator=gen) / 16).to(DEV)
        self.w_gen = (torch.randn(Wd, 256, generator=gen) / 16).to(DEV)
        self.packs = Fz.LinearGradPacks(self.w_gen, self.w_out)
        assert self.packs.complete()
        self.am = {k: float(getattr(self, k).abs().max()) for k in ("g", "z", "q", "dp", "w_out", "w_gen")}

    def run(self):
        """every destination pre-filled with NaN, the row-shaped ones slices of padded rows"""
        M, Wd = self.M, self.Wd
        am = {k: Fz.absmax_device(getattr(self, k).contiguous()) for k in ("g", "z", "q", "dp")}
        g_img, q_img = Fz.linear_pack_act(self.g, am["g"]), Fz.linear_pack_act(self.q, am["q"])
        dp_img = Fz.linear_pack_act(self.dp, am["dp"])
        wt_out, wt_gen = self.packs.transposed("out"), self.packs.transposed("gen")
        nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
        dz_rows, dq_rows = nan(M, Wd + 4), nan(M, 256 + 8)
        r = {}
        r["dZ"] = Fz.generator_ds(g_img, wt_out[0], None, wt_out[1], am["g"], out=dz_rows[:, :Wd])
        r["dquery"] = Fz.linear_reduce(Fz.outproj_fused(dp_img, wt_gen[0], Fz.outproj_slices(Wd)), None, am["dp"], wt_gen[1],
                                       out=dq_rows[:, :256])
        r["dW_out"] = Fz.linear_wgrad(g_img, am["g"], self.z, am["z"], False, out=nan(256, Wd))
        r["dW_gen"], r["db_gen"] = Fz.linear_wgrad(q_img, am["q"], self.dp, am["dp"], True, colsum=True, out=nan(Wd, 256))
        r["db_out"] = self.g.sum(0)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dz_rows[:, Wd:]).all()) and bool(torch.isnan(dq_rows[:, 256:]).all()), "written past a row's width"
        return r

    def reference(self, drop=None):
        """name -> (float64 reference, A, the library's fp32 result); ``drop``: one index of every reduction left out"""
        d = lambda x: x.double()  # noqa: E731
        g, z, q, dp, wo, wg = d(self.g), d(self.z), d(self.q), d(self.dp), d(self.w_out), d(self.w_gen)
        keep = lambda n: torch.arange(n, device=DEV) != (-1 if drop is None else drop % n)  # noqa: E731
        am = self.am
        km, kn, kw = keep(self.M), keep(256), keep(self.Wd)
        out = {}
        out["dZ"] = bound_A(g[:, kn], wo[kn], am["g"], am["w_out"]) + (self.g @ self.w_out,)
        out["dquery"] = bound_A(dp[:, kw], wg[kw], am["dp"], am["w_gen"]) + (self.dp @ self.w_gen,)
        out["dW_out"] = bound_A(g[km].t(), z[km], am["g"], am["z"]) + (self.g.t() @ self.z,)
        out["dW_gen"] = bound_A(dp[km].t(), q[km], am["dp"], am["q"]) + (self.dp.t() @ self.q,)
        out["db_gen"] = (dp[km].sum(0), dp[km].abs().sum(0), self.dp.sum(0))
        out["db_out"] = (g[km].sum(0), g[km].abs().sum(0), None)
        return out


@pytest.mark.parametrize("Wd", [128, 384, 4608])
@pytest.mark.parametrize("M", [1, 17, 33, 130])
def test_products_against_float64(M, Wd):
    c = Case(M, Wd)
    got, ref = c.run(), c.reference()
    for name, (r, A, lib) in ref.items():
        check(name, got[name], r, A, lib)
    wrong = c.reference(drop=M // 2 + 3)
    for name, (r, _, _) in wrong.items():
        assert fails(got[name], r, ref[name][1]), f"M{M} Wd{Wd}: {name} does not see a dropped index of its reduction"


@pytest.mark.parametrize("factor", [3e7, 1e-9])
def test_gradient_scale(factor):
    """the gradients (g, dP) times ``factor``: the scaled results within the same bound (A scales along)"""
    c = Case(33, 384, gscale=factor)
    got, ref = c.run(), c.reference()
    for name, (r, A, _) in ref.items():
        check(name + f" x{factor:g}", got[name], r, A)


def test_zero_gradient_gives_exact_zeros():
    c = Case(17, 384, gscale=0.0)
    for name, v in c.run().items():
        assert float(v.abs().max()) == 0.0, name


# ------------------------------------------------------------------------------------------------ the module
def _module(E, P, G, sd=None):
    m = T.AdaptiveMixing(in_dim=E, in_points=P, n_groups=G, query_dim=256, out_points=128).eval()
    if sd is not None:
        m.load_state_dict(sd)
    return m.to(DEV)


def _pad_last(a, n=256):
    return torch.cat([a, a.new_zeros(a.shape[:-1] + (n - a.shape[-1],))], dim=-1)


def test_module_gradients_match_the_reference(golden_dir, switch_on):
    """fails before AdaptiveMixing.forward_train existed.  The fixture (query_dim 4) embedded in query_dim 256 by zero padding."""
    g = np.load(os.path.join(golden_dir, "mixing_grad_small.npz"))
    P, G = int(g["in_points"]), int(g["n_groups"])
    QD = g["query"].shape[-1]
    sd = {"parameter_generator.weight": _pad_last(t(g["w:parameter_generator.weight"]).float()),
          "parameter_generator.bias": t(g["w:parameter_generator.bias"]).float(),
          "out_proj.weight": _pad_last(t(g["w:out_proj.weight"]).float().t()).t().contiguous(),
          "out_proj.bias": _pad_last(t(g["w:out_proj.bias"]).float())}
    m = _module(64 * G, P, G, sd)
    x = t(g["x"]).to(DEV).requires_grad_()
    query = _pad_last(t(g["query"])).to(DEV).requires_grad_()
    assert m.linear_grad_supported(x, query) and m.linear_grad_packs() is not None
    out = m.forward_train(x, query)
    (out * _pad_last(t(g["gout"])).to(DEV)).sum().backward()
    p = dict(m.named_parameters())
    got = {"out": out[..., :QD], "x": x.grad, "query": query.grad[..., :QD],
           "parameter_generator.weight": p["parameter_generator.weight"].grad[:, :QD],
           "parameter_generator.bias": p["parameter_generator.bias"].grad,
           "out_proj.weight": p["out_proj.weight"].grad[:QD], "out_proj.bias": p["out_proj.bias"].grad[:QD]}
    worst = {}
    for k, v in got.items():
        want = t(g["out" if k == "out" else "g:" + k]).double()
        worst[k] = ((v.detach().cpu().double() - want).abs().max() / want.abs().max()).item()
    print("\nmodule (split-precision Linears) vs reference golden, max |err| / max |value|:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) < 2e-5, worst
    # the padding is an exact embedding: zero weights and zero gouts give exact zeros
    assert float(query.grad[..., QD:].abs().max()) == 0.0 and float(p["parameter_generator.weight"].grad[:, QD:].abs().max()) == 0.0
    assert float(p["out_proj.weight"].grad[QD:].abs().max()) == 0.0 and float(p["out_proj.bias"].grad[QD:].abs().max()) == 0.0


def _drawn(m64, G, P, Q, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(1, Q, G, P, 64, generator=gen).to(DEV)
    query = torch.randn(1, Q, 256, generator=gen).to(DEV)
    for _ in range(60):     # redraw the queries with a pre-activation closer than MARGIN to zero
        with torch.no_grad():
            bad = (min_margin(x, m64.parameter_generator(query.double()), P, G).reshape(Q, G) < MARGIN).any(-1)
        if not bool(bad.any()):
            break
        idx = bad.nonzero().flatten().cpu()
        x[0, idx] = torch.randn(len(idx), G, P, 64, generator=gen).to(DEV)
        query[0, idx] = torch.randn(len(idx), 256, generator=gen).to(DEV)
    else:
        raise AssertionError("could not draw inputs clear of the ReLU kinks")
    return x, query, torch.randn(1, Q, 256, generator=gen).to(DEV)


@pytest.mark.parametrize("G,P,Q", [(1, 4, 21), (4, 7, 33)])
def test_module_against_the_float64_torch_path(G, P, Q, switch_on):
    torch.manual_seed(5 + G)
    m = _module(64 * G, P, G)
    m64 = _module(64 * G, P, G, {k: v.double() for k, v in m.state_dict().items()}).double()
    x, query, gout = _drawn(m64, G, P, Q, 6 + P)
    xg, qg = x.clone().requires_grad_(), query.clone().requires_grad_()
    out = m.forward_train(xg, qg)
    (out * gout).sum().backward()
    x64, q64 = x.double().requires_grad_(), query.double().requires_grad_()
    out64 = m64(x64, q64)
    (out64 * gout.double()).sum().backward()
    p64 = dict(m64.named_parameters())
    pairs = [("out", out.detach(), out64.detach()), ("x", xg.grad, x64.grad), ("query", qg.grad, q64.grad)]
    pairs += [(k, p.grad, p64[k].grad) for k, p in m.named_parameters()]
    worst = {}
    for k, got, want in pairs:
        assert got is not None, k
        worst[k] = ((got.double() - want).abs().max() / want.abs().max()).item()
    print(f"\nG{G} P{P} Q{Q} module vs float64 torch path, max |err| / max |value|:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(worst.values()) < 2e-5, worst


def _count(monkeypatch, names):
    calls = {n: 0 for n in names}
    for n in names:
        real = getattr(Fz, n)

        def wrapped(*a, _n=n, _real=real, **k):
            calls[_n] += 1
            return _real(*a, **k)

        monkeypatch.setattr(Fz, n, wrapped)
    return calls


def _small_run(m, x, query, gout, x_grad=True, q_grad=True):
    m.zero_grad(set_to_none=True)
    xg, qg = x.clone().requires_grad_(x_grad), query.clone().requires_grad_(q_grad)
    out = m.forward_train(xg, qg)
    (out * gout).sum().backward()
    torch.cuda.synchronize()
    return [out.detach(), xg.grad, qg.grad] + [p.grad for p in m.parameters()]


def test_backward_reproducible_and_unasked_gradients_skipped(monkeypatch, switch_on):
    G, P, Q = 4, 7, 33
    torch.manual_seed(3)
    m = _module(64 * G, P, G)
    gen = torch.Generator().manual_seed(4)
    x, query = torch.randn(1, Q, G, P, 64, generator=gen).to(DEV), torch.randn(1, Q, 256, generator=gen).to(DEV)
    gout = torch.randn(1, Q, 256, generator=gen).to(DEV)
    a, b = _small_run(m, x, query, gout), _small_run(m, x, query, gout)
    for u, v in zip(a, b):
        assert torch.equal(u, v), "two runs differ"
    calls = _count(monkeypatch, ["linear_wgrad", "generator_ds", "outproj_fused", "pack_linear_weight_t"])
    _small_run(m, x, query, gout)
    # forward: one generator launch, one out_proj launch; backward: dZ on the generator kernel, dquery on the out_proj kernel, two
    # weight gradients; the transposed packs were made by the runs before (same weight version)
    assert calls == dict(linear_wgrad=2, generator_ds=2, outproj_fused=2, pack_linear_weight_t=0), calls
    for p in m.parameters():
        p.requires_grad_(False)
    for k in calls:
        calls[k] = 0
    r = _small_run(m, x, query, gout)
    assert calls["linear_wgrad"] == 0 and calls["generator_ds"] == 2 and calls["outproj_fused"] == 2, calls
    assert torch.equal(r[1], a[1]) and torch.equal(r[2], a[2]) and all(g is None for g in r[3:])
    # weights trainable, inputs not: the generator's data gradient (the out_proj kernel's second launch) is skipped; dZ is still
    # needed, by the mixing core's parameter gradient
    for p in m.parameters():
        p.requires_grad_(True)
    for k in calls:
        calls[k] = 0
    r = _small_run(m, x, query, gout, x_grad=False, q_grad=False)
    assert calls == dict(linear_wgrad=2, generator_ds=2, outproj_fused=1, pack_linear_weight_t=0), calls
    assert r[1] is None and r[2] is None and all(torch.equal(u, v) for u, v in zip(r[3:], a[3:]))
    # a weight update is a new version: packed again, once per image
    with torch.no_grad():
        m.out_proj.weight.mul_(1.5)
    for k in calls:
        calls[k] = 0
    _small_run(m, x, query, gout)
    assert calls["pack_linear_weight_t"] == 2, calls


def test_switch_off_is_the_route_of_before():
    """same inputs, two routes in one test: forward_train with the switch off against forward on a live split, bit for bit"""
    assert T.AdaptiveMixing.fused_linear_grad in (False, True)
    G, P, Q = 4, 7, 33
    torch.manual_seed(8)
    m = _module(64 * G, P, G)
    m.fused_linear_grad = False
    gen = torch.Generator().manual_seed(9)
    x, query = torch.randn(1, Q, G, P, 64, generator=gen).to(DEV), torch.randn(1, Q, 256, generator=gen).to(DEV)
    gout = torch.randn(1, Q, 256, generator=gen).to(DEV)
    a = _small_run(m, x, query, gout)
    m.zero_grad(set_to_none=True)
    xg, qg = x.clone().requires_grad_(), query.clone().requires_grad_()
    out = m(xg, qg, m.split_out_proj())
    (out * gout).sum().backward()
    b = [out.detach(), xg.grad, qg.grad] + [p.grad for p in m.parameters()]
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    with torch.no_grad():       # no_grad: the switch does not matter
        m.fused_linear_grad = True
        assert torch.equal(m.forward_train(x, query), m(x, query, m.split_out_proj()))


# ------------------------------------------------------------------------------------------------ the decoder layer
def test_decoder_layer_within_the_fixture_bound(golden_dir, switch_on):
    g = DR.load_golden(golden_dir)
    layer = DR.build_layer(g, device=DEV)
    calls = []
    real = T.split_generator_forward
    try:
        T.split_generator_forward = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
        out, grads = DR.run_layer(layer, g, device=DEV)
    finally:
        T.split_generator_forward = real
    assert calls, "the training route did not take the split-precision Linears"
    report = []
    bad = DR.check_against_golden(g, out, grads, "training route, split-precision mixing Linears", report)
    worst = sorted(report, key=lambda r: -r[1] / r[3])[:8]
    print("\nclosest to the bound:", ", ".join(f"{k} {e:.1e} (ref {r:.1e})" for k, e, r, _ in worst))
    assert not bad, "\n".join(bad)


def _two_layers(layer, g):
    """two chained calls of the layer (the second on the first's features and refined boxes), the fixture's gouts on the second"""
    tt = lambda k: torch.from_numpy(np.asarray(g[k]).astype(np.float32)).to(DEV)  # noqa: E731
    leaves = {k: tt(k).requires_grad_() for k in ("query_bbox", "query_feat", "lss", "radar")}
    feats = [tt(f"feat{i}").requires_grad_() for i in range(len(DR.HWS))]
    td_safe = tt("time_diff").clone()
    td_safe[td_safe < 1e-5] = 1.0
    metas = [dict(img_shape=[(DR.IMG_HW[0], DR.IMG_HW[1], 3)], time_diff=tt("time_diff"), lidar2img=tt("lidar2img"), time_diff_safe=td_safe)]
    layer.zero_grad(set_to_none=True)
    layer._carry = None
    feat, cls, pred = layer(leaves["query_bbox"], leaves["query_feat"], feats, leaves["lss"], leaves["radar"], None, metas, layer=DR.LAYER)
    feat, cls, pred = layer(pred, feat, feats, leaves["lss"], leaves["radar"], None, metas, layer=DR.LAYER + 1)
    ((feat * tt("gout_feat")).sum() + (cls * tt("gout_cls")).sum() + (layer.last_bbox_xy * tt("gout_xy")).sum()).backward()
    torch.cuda.synchronize()
    grads = {"p:" + k: p.grad for k, p in layer.named_parameters()}
    grads.update({k: v.grad for k, v in leaves.items()})
    grads.update({f"feat{i}": f.grad for i, f in enumerate(feats)})
    return [feat.detach(), cls.detach(), pred.detach()], grads


def test_decoder_two_layers_reproducible(golden_dir, switch_on):
    """bitwise equal over two runs wherever tests/test_decoder_grad_gpu.py holds the training route to that: everything except what
    atomic scatters feed (the pyramid levels, the BEV streams and what lies upstream of them), 1e-5 of the largest element there"""
    g = DR.load_golden(golden_dir)
    layer = DR.build_layer(g, device=DEV)
    _two_layers(layer, g)       # (the process's first pass through the library's GEMMs selects their algorithms)
    o1, g1 = _two_layers(layer, g)
    o2, g2 = _two_layers(layer, g)
    for a, b in zip(o1, o2):
        assert torch.equal(a, b)
    scattered = ("feat", "lss", "radar", "p:sampling_radar_bev.temporal_encoder.", "p:sampling_radar_bev.attention.value_proj.",
                 "p:sampling_lss_bev.attention.value_proj.", "p:sampling_radar_bev.positional_encoding.",
                 "p:sampling_lss_bev.positional_encoding.")
    for name, a in g1.items():
        assert a is not None, name
        if name.startswith(scattered):
            assert float((a - g2[name]).abs().max()) <= 1e-5 * float(a.abs().max()), name
        else:
            assert torch.equal(a, g2[name]), f"{name}: two runs differ"
