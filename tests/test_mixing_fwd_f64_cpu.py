"""The float64 criterion of tests/test_mixing_fwd_f64_gpu.py without a GPU: every case of tests/mixing_fwd_ref.py with the
restatements standing in for the kernels (float32 torch for the f32 mode, the model of the split-precision operand handling for
f16x3).  What this shows here: every reference passes its own bound, the representation term R included; each negative control
-- the restatement with one deliberate fault -- fails its check on a case the restatement alone passes; the model of the f16x3
kernel, which splits S as it is, meets the sweep with R's 2^-25 floor and misses it without at small std(S); the host forms of
rac_split_f16 and mix_split_bf16 do what the kernel's do; and rac_mixing_fwd / mixing_fused refuse what they must before anything
is launched."""
import ctypes

import pytest
import torch

import mixing_fwd_ref as W
from racformer_amd import _lib, fused

RUN = W.Restated()
NAN = float("nan")


@pytest.fixture(scope="module")
def log():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield W.Log()
    torch.set_num_threads(n)


# ------------------------------------------------------------------------------------------------------------ every check
@pytest.mark.parametrize("mode", W.MODES)
@pytest.mark.parametrize("name", W.PLAIN)
def test_case(log, name, mode):
    W.check_case(log, name, RUN, mode)


@pytest.mark.parametrize("mode", W.MODES)
@pytest.mark.parametrize("name", W.POISON)
def test_poisoned_items(log, name, mode):
    W.check_poison(log, name, RUN, mode)


@pytest.mark.parametrize("name", W.SWEEP)
def test_s_magnitude_sweep(log, name):
    W.check_case(log, name, RUN, "f16x3")
    e = log.errors[f"f16x3 | {name} | out"]
    assert {"E_ref", "kernel", "allowed", "ratio"} <= set(e) and e["ratio"] <= 1


def test_small_S_is_as_accurate_as_its_representation_and_no_better():
    """the f16x3 kernel's known limit: S is split as it is, so below |S| = 2^-3 its lo half is an f16 subnormal and S carries an
    absolute error of 2^-25 that the second LayerNorm magnifies.  The model meets R with that floor at every k (above) and
    misses R without it at std(S) = 2^-12 (at P = 7 from 2^-8 down), where the recorded ratio says by how much."""
    for P, ks in ((96, (-12,)), (7, (-12, -10, -8))):
        for k in ks:
            with pytest.raises(W.OutOfBound):
                W.check_case(W.Log(), f"sweep k{k} P{P}", RUN, "f16x3", s_floor="none")
        lg = W.Log()
        W.check_case(lg, f"sweep k-12 P{P}", RUN, "f16x3")
        e = lg.errors[f"f16x3 | sweep k-12 P{P} | out"]
        assert e["ratio"] <= 1 < e["ratio_without_floor"] < e["ratio_absent"]
        W.check_case(lg, f"sweep k0 P{P}", RUN, "f16x3", s_floor="none")


# -------------------------------------------------------------------------------------------- what the cases are named for
def test_cases_cover_what_they_are_named_for():
    specs = W.CASES
    assert {s["P"] for n, s in specs.items() if n in W.PLAIN} >= set(W.P_LIST) and len(W.P_LIST) == 18
    assert all(3 <= s["N"] <= 6 and s["G"] in (1, 4) for s in specs.values())
    assert {s["G"] for n, s in specs.items() if n.startswith("P")} == {1, 4}
    assert {(s["P"], s.get("ps", 1.0)) for s in specs.values() if s.get("stats")} == {(P, ps) for P in (96, 7) for ps in (1.0, 2.0 ** -6)}
    assert any(s.get("ld") and s.get("ps", 1.0) != 1.0 for s in specs.values())
    assert {(s["P"], s["period"] * 2 == s["N"] or s["period"]) for s in specs.values() if "period" in s} == {(96, True), (96, 1), (7, True), (7, 1)}
    assert len(W.SWEEP) == 18 and {W.CASES[n]["s_std"] for n in W.SWEEP} == {2.0 ** k for k in range(-12, 5, 2)}
    assert any(not W.build(n)["guard"] for n in W.PLAIN) and sum(W.build(n)["guard"] for n in W.PLAIN) > len(W.PLAIN) // 2
    for name in W.PLAIN + W.POISON:                    # every item has contents of its own
        c = W.build(name)
        flat = c["x"].nan_to_num(nan=7.0, posinf=8.0).reshape(c["N"] * c["G"], -1)
        assert len({tuple(r[:8].tolist()) for r in flat}) == len(flat) or name.startswith("stats")
        assert c["params"].stride(-1) == 1 and c["params"].stride(-2) % 4 == 0 and c["off"] % 4 == 0
        assert (c["params"].stride(-2) > c["width"]) == bool(specs[name].get("ld"))
    # the statistics items are what they are called
    c, ref = W.build("stats P96 ps1"), W.reference("stats P96 ps1")
    rows = c["params"].reshape(6, -1)
    f = W.MR.forward64(c["x"], rows.double().view(1, 6, -1), 96, 4)
    var = lambda t: float(t.var(unbiased=False))        # noqa: E731
    n, g = W.STAT_ITEMS["zero"]
    assert bool((ref["A"][n, g] == 0).all()) and bool((ref["Z"][n, g] == 0).all())
    n, g = W.STAT_ITEMS["eps"]
    assert 0.3 * W.EPS < var(f["A"][n, g]) < 3 * W.EPS
    n, g = W.STAT_ITEMS["offset"]
    assert abs(float(f["A"][n, g].mean()) - 1e3) < 1 and 0.3 < var(f["A"][n, g]) < 3
    n, g = W.STAT_ITEMS["outlier"]
    assert float(f["A"][n, g].abs().max()) > 100 * float(f["A"][n, g].abs().median())
    assert var(f["A"][0, 1]) > 1e10 and var(f["A"][0, 2]) < 1e-9 and var(f["A"][5, 2]) < 1e-9
    # the poisoned items: one non-finite input each
    c = W.build("poison P7")
    assert int((~torch.isfinite(c["x"])).sum()) == 2 and int(torch.isnan(c["params"]).sum()) == 2 and c["ps"] == 1.0
    per = 4096 + 128 * 7
    n, g = W.POISON_ITEMS["nan in S"]
    S = c["params"].reshape(6, 4, per)[n, g, 4096:].view(128, 7)
    assert int(torch.isnan(S[:, 6]).sum()) == 1 and int(torch.isnan(S).sum()) == 1
    assert bool(torch.isfinite(c["clean"][0]).all()) and bool(torch.isfinite(c["clean"][1]).all())


def test_magnitude_bounds_the_value_on_non_negative_input_and_R_grows_with_its_floor():
    ref = W.reference("P33")
    assert bool((ref["A"] >= ref["Z"].abs()).all())
    assert bool((ref["R"]["fixed"] >= ref["R"]["none"]).all())
    small, unit = W.reference("sweep k-12 P96")["R"], W.reference("sweep k0 P96")["R"]
    assert float((small["fixed"] / small["none"]).min()) > 10 and float((unit["fixed"] / unit["none"]).max()) < 1.01


# ------------------------------------------------------------------------------------------ host forms of the helpers
def test_host_split_helpers():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(4096, generator=g) * torch.logspace(-6, 3, 4096)
    hi, lo = W.split_f16(v)
    err = (hi.double() + lo.double() - v.double()).abs()
    assert bool((err <= torch.clamp(2.0 ** -22 * v.double().abs(), min=2.0 ** -25)).all())
    assert float((err / v.double().abs())[v.abs() < 2.0 ** -10].max()) > 2.0 ** -18      # (the floor is what binds for small values)
    t1, t2, t3 = W.split_bf16(v)
    assert torch.equal((t1.double() + t2.double() + t3.double()).float(), v)
    assert all(torch.equal(t.bfloat16().float(), t) for t in (t1, t2, t3))
    z = torch.arange(128.0).view(2, 64) / 7
    img = W.split_image(z)
    assert tuple(img.shape) == (2, 2, 64) and torch.equal(img[1, 1, :32], (z[1, 32:] * 16).half())
    assert torch.equal(img[0, 0, 32:], (z[0, :32] * 16 - (z[0, :32] * 16).half().float()).half())


# ------------------------------------------------------------------------------------------------------- negative controls
def _case(name, mode, items=None):
    return lambda log, run: W.check_case(log, name, run, mode, items=items)


def _poison(name, mode):
    return lambda log, run: W.check_poison(log, name, run, mode)


EPS_ITEM = [W.STAT_ITEMS["eps"]]
CONTROLS = {"ln1_over_padded_rows": [_case("P1", "f32"), _case("P33", "f32"), _case("P95", "f16x3")],
            "s_last_column_dropped": [_case("P7", "f32"), _case("P7", "f16x3")],
            "param_row_q_div_period": [_case("period half P96", "f32"), _case("period half P7", "f16x3")],
            "group_offset_with_P96": [_case("P7", "f32"), _case("stats P7 ps1", "f16x3")],
            "unbiased_variance": [_case("P96", "f32"), _case("P17", "f16x3")],
            "eps_dropped": [_case("stats P96 ps1", "f32", EPS_ITEM), _case("stats P7 ps1", "f16x3", EPS_ITEM)],
            # (LayerNorm hides a common factor of A except through eps)
            "param_scale_not_on_M": [_case("stats P96 ps0.015625", "f32", EPS_ITEM), _case("stats P7 ps0.015625", "f16x3", EPS_ITEM)],
            "hi_lo_dropped": [_case("P96", "f16x3"), _case("P7", "f16x3"), _case("sweep k0 P96", "f16x3")],
            "relu_drops_nan": [_poison("poison P7", "f32"), _poison("poison P7", "f16x3"), _poison("poison P96", "f32"),
                               _poison("poison P96", "f16x3")]}


@pytest.mark.parametrize("fault", W.FAULTS)
def test_negative_control_fails_its_check(fault):
    assert set(CONTROLS) == set(W.FAULTS)
    for check in CONTROLS[fault]:
        check(W.Log(), RUN)                                            # the same check passes without the fault
        with pytest.raises(W.OutOfBound):
            check(W.Log(), W.Restated(fault))


# ------------------------------------------------------------------------------------------------------------- refusals
def _lib_or_fail():
    try:
        return _lib.lib()
    except RuntimeError as e:
        pytest.fail(str(e))


def test_mixing_fwd_argument_errors():
    """the argument checks of rac_mixing_fwd / rac_mixing_period_fwd run before any HIP call"""
    lib = _lib_or_fail()
    d = ctypes.c_void_p(16)                     # never dereferenced: every failing call below fails its checks first
    P, G = 13, 2
    Wd = G * (4096 + 128 * P)

    def last():
        return lib.rac_last_error().decode()

    def fwd(nq=6, G=G, P=P, C=64, out=128, ld=Wd, mode=_lib.MIX_F32, x=d, o=d, o16=None, period=None):
        head = (x, x, 1.0, o, o16, 16.0, ld)
        tail = (nq, G, P, C, out, 1e-5, mode, None)
        return lib.rac_mixing_fwd(*head, *tail) if period is None else lib.rac_mixing_period_fwd(*head, period, *tail)

    for mode in (_lib.MIX_F32, _lib.MIX_F16X3):
        assert fwd(C=32, mode=mode) == -1 and "64 channels" in last() and "rac_mixing_fwd" in last()
        assert fwd(out=64, mode=mode) == -1 and "128 out points" in last()
        assert fwd(P=0, mode=mode) == -1 and "in_points=0" in last()
        assert fwd(P=97, ld=2 * (4096 + 128 * 97), mode=mode) == -1 and "in_points=97" in last()
        assert fwd(nq=-1, mode=mode) == -1 and "bad sizes" in last()
        assert fwd(G=0, mode=mode) == -1 and "bad sizes" in last()
        assert fwd(ld=Wd - 4, mode=mode) == -1 and "parameter row stride" in last()
        assert fwd(ld=Wd + 2, mode=mode) == -1 and "parameter row stride" in last()      # not a multiple of 4 (float4 staging)
        for period in (0, 4, 7, 12):
            assert fwd(period=period, mode=mode) == -1 and f"period {period} does not divide 6 rows" in last()
        assert fwd(x=None, mode=mode) == -1 and "null pointer" in last()
        assert fwd(o=None, o16=None, mode=mode) == -1 and "null pointer" in last()
        assert fwd(nq=0, x=None, o=None, mode=mode) == 0          # empty: nothing to check or launch
    assert fwd(mode=7) == -1 and "mfma_mode=7" in last()


def test_mixing_fused_refuses_host_tensors():
    """well-sized operands off the GPU: refused as such, nothing launched and nothing computed in torch instead"""
    x, params = torch.zeros(1, 3, 2, 5, 64), torch.zeros(1, 3, 2 * (4096 + 128 * 5))
    for kw in (dict(), dict(f16x3=True), dict(split=True), dict(period=1)):
        with pytest.raises(RuntimeError, match="CUDA"):
            fused.mixing_fused(x, params, 5, 2, **kw)
