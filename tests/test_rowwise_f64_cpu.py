"""The float64 criterion of tests/test_rowwise_f64_gpu.py without a GPU: every case of tests/rowwise_ref.py with the float32
restatement standing in for the kernels.  What this shows here: every reference passes its own bound (finite magnitudes, E_ref
finite, the sentinel and bit-equality checks hold for a correct implementation); each negative control -- the restatement with
one deliberate fault: the issue's eleven and a ReLU that drops a NaN -- fails its check; the launcher rules the GPU module restates select what the cases are
named for; and the Python wrappers refuse mis-sized operands by name, on any device, before anything is launched."""
import types

import pytest
import torch

import rowwise_ref as W
from racformer_amd import fused

RUN = W.Restated32()


@pytest.fixture(scope="module")
def log():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield W.Log()
    torch.set_num_threads(n)


# ------------------------------------------------------------------------------------------------------------ every check
@pytest.mark.parametrize("name", list(W.ROWGEMM_CASES))
def test_rowgemm_case(log, name):
    W.check_rowgemm(log, name, W.rowgemm_build(name), RUN)


@pytest.mark.parametrize("name", list(W.ADD_LN_CASES))
def test_add_ln_case(log, name):
    W.check_add_ln(log, name, W.add_ln_build(name), RUN)


@pytest.mark.parametrize("rows", W.SIZES + (74,))
def test_pe_head_case(log, rows):
    W.check_pe_head(log, f"rows{rows}", W.pe_case(50 + rows, rows), RUN)
    if rows == 5:
        W.check_pe_head(log, "rows5 W=0", W.pe_case(49, rows, zero_weight=True), RUN)
        W.check_pe_head(log, "rows5 NaN row", W.pe_case(48, rows, nan_row=2), RUN)


@pytest.mark.parametrize("boundary", [False, True], ids=["refine", "layer_boundary"])
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("shape", list(W.REFINE_SHAPES))
def test_refine_case(log, shape, T, boundary):
    B, Q = W.REFINE_SHAPES[shape]
    W.check_refine(log, f"{shape} T{T}", W.refine_case(60 + 7 * B * Q + T, B, Q, T), RUN, boundary)


@pytest.mark.parametrize("boundary", [False, True], ids=["refine", "layer_boundary"])
def test_refine_beside_poisoned_rows(log, boundary):
    c = W.refine_case(77, 2, 37, 3, poison=True)
    assert len(c["poisoned"]) == 2
    W.check_refine(log, "B2 Q37 T3 poisoned", c, RUN, boundary)


@pytest.mark.parametrize("name", list(W.GRU_CASES))
def test_gru_gate_case(log, name):
    W.check_gru(log, name, W.gru_case(name), RUN)


@pytest.mark.parametrize("name", list(W.UPSAMPLE_CASES))
def test_upsample2x_case(log, name):
    W.check_upsample(log, name, W.upsample_case(name), RUN)


# -------------------------------------------------------------------------------------------- what the cases are named for
def test_cases_reach_the_paths_they_are_named_for():
    rg = W.ROWGEMM_CASES
    assert {c[0] for c in rg.values()} >= {1, 15, 16, 17, 37, 81}
    assert {len(gm[4]) for c in rg.values() for gm in c[1]} == {1, 2, 3} and {len(c[1]) for c in rg.values()} == {1, 2, 3}
    assert {gm[0] for c in rg.values() for gm in c[1]} >= {1, 10, 63, 64, 65, 512, 2189}
    assert {s.get("P", 1) for c in rg.values() for gm in c[1] for s in gm[4]} >= {1, 2, 3, 4, 5, 16}
    for name, want in W.ROWGEMM_INSTANTIATION.items():
        rows, gemms = rg[name][0], rg[name][1]
        assert W.rowgemm_instantiation(rows, [gm[0] for gm in gemms], len(gemms[0][4])) == want, name
    assert W.rowgemm_instantiation(81, [10, 256, 2189], 1) == (1, 1, False) and W.rowgemm_instantiation(37, [10, 256, 2189], 1) == (1, 1, True)
    ad = W.ADD_LN_CASES
    for name, c in ad.items():
        assert W.add_ln_kernel(c["dim"], c["P"]) == c["kernel"] == name.split()[0], name
    assert W.add_ln_kernel(256, 7) == "simple" and W.add_ln_kernel(256, 8) == "many" and W.add_ln_kernel(512, 32) == "simple"
    assert {c["rows"] for c in ad.values()} >= {1, 3, 4, 5, 205}
    assert {(c["dim"], c["P"]) for c in ad.values()} >= {(d, s) for d in (4, 100, 256, 260, 512, 1024) for s in (1, 2, 7)} | \
        {(256, s) for s in (8, 9, 13, 16, 32)}
    for kernel in ("simple", "many"):
        mine = [c for c in ad.values() if c["kernel"] == kernel]
        assert {c["split"] for c in mine} == {None, "lines", "kcat"} and any(c["post"] for c in mine) and any(c["relu"] for c in mine)
        assert any(c["scale"] != 1.0 for c in mine) and any(c["out_slice"] for c in mine) and any(c.get("stats") for c in mine)
    assert any(c["P"] % 4 for c in ad.values() if c["kernel"] == "many") and any(c["ld"] for c in ad.values())
    assert [W.grid_stride("gru_gate", W.gru_case(n)["items"]) for n in W.GRU_CASES] == [False] * 5 + [True]
    assert W.gru_case("past the cap")["items"] == 1064960
    assert [W.grid_stride("upsample2x", W.upsample_case(n)["items"]) for n in W.UPSAMPLE_CASES] == [False] * 5 + [True]
    assert W.upsample_case("past the cap")["items"] == 2129920
    assert len(W.TEMPLATES) * 2 <= 2 * 37 and len(W.FAULTS) == 12
    # the 2 x 37 refine case holds every edge row: both clamps of x and of y active, every inverse_sigmoid edge, both batches' times
    c = W.refine_case(60 + 7 * 74 + 3, 2, 37, 3)
    pred, xy, table = W.refine_forward(c, W.F64)
    for col in (0, 1):
        assert bool((xy[..., col] == 0).any()) and bool((xy[..., col] == 1).any())
    for col in (1, 2):
        assert {float(torch.tensor(v, dtype=torch.float32)) for v in W.EDGE} <= set(c["prop"][..., col].flatten().tolist())
    assert float(pred[..., 0].min()) < 0 and float(pred[..., 0].max()) > 1 and float(c["delta"][..., :3].abs().max()) == 30
    assert bool(((c["delta"][..., 6] == 0) & (c["delta"][..., 7] == 0)).any()) and float(c["delta"][..., 3:6].abs().max()) == 5
    assert float(c["td"][0, 1]) != float(c["td"][1, 1])


def test_upsample64_is_torch_in_float64_and_magnitude_is_plain_on_non_negative_input():
    for name in ("1x2", "3x4", "20x12 planes5"):
        x = W.upsample_case(name)["x"]
        ref = torch.nn.functional.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=True)
        # (torch rounds the ratio before it multiplies: a tap position a few 2^-53 of the map size off)
        assert float((W.upsample64(x) - ref).abs().max()) < 1e-12
        assert torch.equal(W.upsample64(x.abs()), W.upsample64(x, magnitude=True))
    s = W.add_ln_build("simple dim256 S7")
    for k in ("a", "bias0", "res", "gamma", "beta", "post"):
        if s[k] is not None:
            s[k].abs_()
    assert bool((W.pro_mag(s) >= W.pro_value(s, W.F64).abs() * (1 - 1e-12)).all())


def test_split_image_layouts():
    x = torch.randn(3, 64)
    k, l = W.split_image(x, "kcat"), W.split_image(x, "lines")
    assert tuple(k.shape) == (3, 3 * 64 + 64) and tuple(l.shape) == (3, 128)
    hi = (x * 16).half()
    assert torch.equal(k[:, :64], hi) and torch.equal(k[:, 64:128], hi) and torch.equal(l[:, :32], hi[:, :32]) and torch.equal(l[:, 64:96], hi[:, 32:])
    assert torch.equal(l[:, 32:64], k[:, 128:160]) and torch.equal(k[:, 192:], torch.tensor([16.0, 16.0] + [0.0] * 62).half().expand(3, 64))
    assert float(((hi.double() + k[:, 128:192].double()) / 16 - x.double()).abs().max()) <= 2.0 ** -21 * float(x.abs().max())


# ------------------------------------------------------------------------------------------------------- negative controls
def _rowgemm(name):
    return lambda log, run: W.check_rowgemm(log, name, W.rowgemm_build(name), run)


def _add_ln(name):
    return lambda log, run: W.check_add_ln(log, name, W.add_ln_build(name), run)


def _refine(boundary):
    return lambda log, run: W.check_refine(log, "B2 Q37 T3", W.refine_case(60 + 7 * 74 + 3, 2, 37, 3), run, boundary)


CONTROLS = {"variance_over_dim_minus_1": [_add_ln("simple dim256 S1"), _rowgemm("ln relu post xout r37 N512")],
            "eps_dropped": [_add_ln("simple statistics S1"), _add_ln("many statistics S8"), _rowgemm("statistics r37 N64")],
            "partial_dropped": [_rowgemm("P3 ln xout relu0 r37 N512"), _add_ln("many dim256 S9")],
            "scale_after_bias": [_rowgemm("P2 scale bias0 r1"), _add_ln("simple dim256 S7"), _add_ln("many dim256 S13")],
            "k_block_dropped": [_rowgemm("plain r15 1seg N64"), _rowgemm("plain r37 3seg N1")],
            "relu_from_off_by_one": [_rowgemm("P2 res ln xout relu256 r15 N512")],
            "residual_next_row": [_rowgemm("res ln kcat r16 N64"), _add_ln("many dim256 S16")],
            "other_batch_time_diff": [_refine(False), _refine(True)],
            "no_eps_clamps": [_refine(False), _refine(True)],
            "align_corners_false": [lambda log, run: W.check_upsample(log, "3x4", W.upsample_case("3x4"), run)],
            "z_swapped": [lambda log, run: W.check_gru(log, "C6 5x7 B2 bias", W.gru_case("C6 5x7 B2 bias"), run)],
            # (beyond the issue's eleven: what fmaxf(NaN, 0) made of a poisoned row before rac_relu)
            "relu_drops_nan": [_rowgemm("nan row relu r37 N65"), _add_ln("simple nan relu S2"), _add_ln("many nan relu S9"),
                               lambda log, run: W.check_pe_head(log, "rows5 NaN row", W.pe_case(48, 5, nan_row=2), run),
                               lambda log, run: W.check_refine(log, "poisoned", W.refine_case(77, 2, 37, 3, poison=True), run, True)]}


@pytest.mark.parametrize("fault", W.FAULTS)
def test_negative_control_fails_its_check(fault):
    assert set(CONTROLS) == set(W.FAULTS)
    for check in CONTROLS[fault]:
        check(W.Log(), RUN)                                            # the same check passes without the fault
        with pytest.raises(W.OutOfBound):
            check(W.Log(), W.Restated32(fault))


# ------------------------------------------------------------------------------------------------------------- refusals
def _norm(dim):
    return types.SimpleNamespace(weight=torch.ones(dim), bias=torch.zeros(dim), eps=1e-5)


def _linear(out=256, k=3):
    return types.SimpleNamespace(weight=torch.zeros(out, k), bias=torch.zeros(out))


def test_add_ln_refuses_mis_sized_operands():
    a = torch.zeros(5, 256)
    for kw, name in ((dict(residual=torch.zeros(4, 256)), "residual"), (dict(residual=torch.zeros(5, 512)), "residual"),
                     (dict(post=torch.zeros(6, 256)), "post"), (dict(bias=torch.zeros(255)), "bias"), (dict(bias=torch.zeros(5, 256)), "bias")):
        with pytest.raises(RuntimeError, match=f"add_ln: {name} "):
            fused.add_ln(a, _norm(256), **kw)
    with pytest.raises(RuntimeError, match="add_ln: norm.weight "):
        fused.add_ln(a, _norm(512))
    with pytest.raises(RuntimeError, match="add_ln: residual "):
        fused.add_ln(torch.zeros(3, 5, 256), _norm(256), residual=torch.zeros(3, 5, 256), num_partials=3)
    with pytest.raises(RuntimeError, match="add_ln: a must be"):
        fused.add_ln(torch.zeros(3, 5, 256), _norm(256), num_partials=2)
    with pytest.raises(RuntimeError, match="add_ln: residual .*float32"):
        fused.add_ln(a, _norm(256), residual=torch.zeros(5, 256, dtype=torch.float64))
    for out in (torch.zeros(4, 256), torch.zeros(5, 260), torch.zeros(5, 512)[:, ::2], torch.zeros(5, 256, dtype=torch.float64)):
        with pytest.raises(RuntimeError, match="add_ln: out "):
            fused.add_ln(a, _norm(256), out=out)
    with pytest.raises(RuntimeError, match="add_ln: out's rows "):
        fused.add_ln(torch.zeros(2, 5, 256), _norm(256), out=torch.zeros(3, 5, 512)[::2, :, :256])
    # well-sized operands off the GPU: refused as such, nothing launched
    for kw in (dict(residual=a), dict(post=a), dict(bias=torch.zeros(256)), dict(out=torch.zeros(5, 256))):
        with pytest.raises(RuntimeError, match="CUDA"):
            fused.add_ln(a, _norm(256), **kw)


def test_row_seg_and_row_gemm_refuse_mis_sized_operands():
    a = torch.zeros(16, 256)
    for kw, name in ((dict(residual=torch.zeros(16, 255)), "residual"), (dict(post=torch.zeros(16, 512)), "post"),
                     (dict(x_out=torch.zeros(16, 260)), "x_out"), (dict(bias0=torch.zeros(128)), "bias0"),
                     (dict(norm=_norm(512)), "norm.weight"), (dict(residual=torch.zeros(256)), "residual")):
        with pytest.raises(RuntimeError, match=f"row_seg: {name} "):
            fused.row_seg(a, **kw)
    with pytest.raises(RuntimeError, match="row_seg: a "):
        fused.row_seg(torch.zeros(16, 512))
    with pytest.raises(RuntimeError, match="row_seg: a "):
        fused.row_seg(torch.zeros(3, 16, 256), num_partials=2)
    norm = _norm(256)
    norm.bias = torch.zeros(255)
    with pytest.raises(RuntimeError, match="row_seg: norm.bias "):
        fused.row_seg(a, norm=norm)
    with pytest.raises(RuntimeError, match="row_gemm: bias "):
        fused.row_gemm([fused.row_seg(a)], torch.zeros(10, 256), torch.zeros(9), torch.zeros(16, 10))
    with pytest.raises(RuntimeError, match="row_gemm: out "):
        fused.row_gemm([fused.row_seg(a)], torch.zeros(10, 256), torch.zeros(10), torch.zeros(16, 12))
    with pytest.raises(RuntimeError, match="row_gemm: weight "):
        fused.row_gemm([fused.row_seg(a), fused.row_seg(a)], torch.zeros(10, 256), None, torch.zeros(16, 10))


def test_rowgemm_launch_refuses_short_operands():
    a, w = torch.zeros(16, 256), torch.zeros(10, 256)
    short = torch.zeros(15, 256)
    for kw, name in ((dict(residual=short), "residual"), (dict(post=short), "post"), (dict(x_out=short), "x_out"),
                     (dict(split_out=torch.zeros(15, 512, dtype=torch.float16), split_lines=True), "split_out")):
        with pytest.raises(RuntimeError, match=f"segment 0: {name} holds 15 rows"):
            fused.rowgemm_launch([fused.row_gemm([fused.row_seg(a, **kw)], w, None, torch.zeros(16, 10))], 16)
    with pytest.raises(RuntimeError, match="segment 1: a holds 15 rows"):
        fused.rowgemm_launch([fused.row_gemm([fused.row_seg(a), fused.row_seg(short)], torch.zeros(10, 512), None, torch.zeros(16, 10))], 16)
    with pytest.raises(RuntimeError, match="segment 0: a holds 5 rows"):
        fused.rowgemm_launch([fused.row_gemm([fused.row_seg(torch.zeros(3, 5, 256), num_partials=3)], w, None, torch.zeros(16, 10))], 16)
    with pytest.raises(RuntimeError, match="GEMM 1: out holds 15 rows"):
        fused.rowgemm_launch([fused.row_gemm([fused.row_seg(a)], w, None, torch.zeros(16, 10)),
                              fused.row_gemm([fused.row_seg(a)], w, None, torch.zeros(15, 10))], 16)
    # well-sized operands off the GPU: refused as such, nothing launched
    with pytest.raises(RuntimeError, match="CUDA"):
        fused.rowgemm_launch([fused.row_gemm([fused.row_seg(a, residual=a)], w, None, torch.zeros(16, 10))], 16)


def test_pe_head_and_layer_boundary_refuse_mis_sized_operands():
    boxes, td = torch.zeros(2, 5, 10), torch.ones(2, 3)
    for lin, norm, name in ((_linear(128), _norm(256), "linear.weight"), (_linear(256, 4), _norm(256), "linear.weight"),
                            (_linear(), _norm(128), "norm.weight")):
        with pytest.raises(RuntimeError, match=f"pe_head: {name} "):
            fused.pe_head(boxes[..., :3], lin, norm)
        with pytest.raises(RuntimeError, match=f"layer_boundary_fused: {name} "):
            fused.layer_boundary_fused(boxes, boxes, td, 150, W.PC, lin, norm)
    lin = _linear()
    lin.bias = torch.zeros(255)
    with pytest.raises(RuntimeError, match="pe_head: linear.bias "):
        fused.pe_head(boxes[..., :3], lin, _norm(256))
    with pytest.raises(RuntimeError, match="pe_head: x3 "):
        fused.pe_head(boxes[..., :4], _linear(), _norm(256))
    for bad in (torch.ones(3, 3), torch.ones(2), torch.ones(2, 3, 1), torch.ones(6)):
        with pytest.raises(RuntimeError, match="layer_boundary_fused: time_diff_safe "):
            fused.layer_boundary_fused(boxes, boxes, bad, 150, W.PC, _linear(), _norm(256))
        with pytest.raises(RuntimeError, match="refine_fused: time_diff_safe "):
            fused.refine_fused(boxes, boxes, bad, 150)
    with pytest.raises(RuntimeError, match="layer_boundary_fused: delta "):
        fused.layer_boundary_fused(boxes, boxes[:, :4], td, 150, W.PC, _linear(), _norm(256))
