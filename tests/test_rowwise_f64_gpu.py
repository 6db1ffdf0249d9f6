"""The decoder's small-launch forward chain on the MI355X against float64, element by element: rac_rowgemm_fwd, rac_add_ln_fwd,
rac_pe_head_fwd, rac_refine_fwd / rac_layer_boundary_fwd, rac_gru_gate_fwd and rac_upsample2x_fwd through the public wrappers of
racformer_amd.fused (tests/rowwise_ref.py holds the cases, references, magnitudes and negative controls;
tests/test_rowwise_f64_cpu.py runs the same checks on the CPU with the float32 restatement in the kernels' place, shows that each
negative control -- the issue's eleven and a ReLU that drops a NaN -- fails its check, and holds the wrappers' refusal tests).

Criterion, per element: |got - ref| <= max(4 x E_ref, 1) x 2^-24 x A; ref the float64 evaluation of the torch / oracle.restate
formulation, E_ref the float32 restatement's own worst err / A on the same case, A the same expression with every term
non-negative; an element with A == 0 is exactly 0; NaN exactly where float64 has NaN.  Every f16 split image is bit-equal to the
split of the rows the kernel wrote beside it; every destination is a region of a larger NaN-filled buffer (extra rows, wider row
stride, neighbouring [:, t] slots) whose remainder must still be NaN.  Every comparison prints its (E_ref, kernel) pair; with
RAC_ROWWISE_ERRORS=<file> the session's pairs are written there as JSON (profiles/rowwise_f64.json is the MI355X run's copy).

Reached, and asserted as reached through the launchers' rules restated in tests/rowwise_ref.py: rowgemm_kernel<1,1,true>,
<1,1,false> (630 workgroups), <2,1,true> and <3,1,true>; rows 1 / 15 / 16 / 17 / 37 / 81; widths 1 .. 2189 with ragged column
slices and three GEMMs of different widths per launch; every prologue the decoder launches; 2, 3, 4, 5 and 16 partials; column-slice
sources and destinations; add_ln_kernel at dims 4 .. 1024 with 1, 2, 7 partials and add_ln_many_kernel with 8, 9, 13, 16, 32; both
split layouts from both; the grid-stride loops of gru_gate and upsample2x; row statistics (constant, offset 1e4, eps-dominated,
outlier, zero, NaN -- in rowgemm's prologue and in both add_ln kernels, with three clean rows in the NaN row's 4-row workgroup)
beside ordinary rows; a NaN row behind a ReLU; refine's clamps, saturating deltas and NaN / inf deltas beside clean rows.

Measured on the MI355X (104 tests in 5.4 s), worst over the session in units of 2^-24 (E_ref | kernel); no comparison above 0.55 of
what max(4 x E_ref, 1) allows:
  rowgemm         2.60 | 2.75  (finished rows; GEMM outputs 2.27 | 2.47, the MFMA chain at K = 256 .. 768)
  add_ln          3.85 | 2.65  (E_ref on the eps-dominated row; the kernel's worst on 205 plain rows)
  pe_head         1.81 | 1.90
  refine          4.12 | 4.12  (xy: the float32 angle, 65 m out; pred 1.31 | 1.47)
  layer_boundary  8.48 | 7.86  (box table, the same angle; pred and xy as refine; pe 2.49 | 2.14)
                  pred, xy, table and pe bit-equal to refine_fused -> box_prep / pe_head in every case (printed, not asserted)
  gru_gate        2.45 | 2.54  (the case past the 4096-workgroup cap)
  upsample2x      with the issue's magnitude 993 | 229 (64 x 64; 462 | 81 past the 8192-workgroup cap, 2.9 | 1.5 at 3 x 4): kernel and
                  torch both form a tap position as float32(ratio) * index, an error that grows with the map and shows in full,
                  relative to A, where the heavier tap holds a value near 0 -- that comparison catches gross indexing errors only on
                  the large maps.  With the position's two roundings carried in the magnitude: 1.41 | 1.65 at every size (64 x 64:
                  0.82 | 0.66; past the cap 1.41 | 1.65), which is the comparison a subtly wrong tap weight fails.
Found by this module and fixed with it: the ReLU of these kernels was fmaxf(v, 0), which turns a NaN into 0 where torch.relu keeps
it -- a poisoned row behind a ReLU prologue or epilogue (rowgemm, add_ln, pe_head, the position-encoder rows of layer_boundary) came
out as clean zeros.  Before: "nan row relu r37 N65", "simple nan relu S2", "many nan relu S9", "rows5 NaN row" and the pe rows of
"B2 Q37 T3 poisoned" each had no NaN in the 256 (512) elements where float64 has one.  rac_relu (rac_common.h) now keeps a NaN and
is fmaxf's bits on every other value, -0 included; after: all five pass, every finite result unchanged (golden, parity and
layer0_once tests untouched and green)."""
import json
import os
import types

import pytest
import torch

import rowwise_ref as W
from racformer_amd import fused

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _norm(gamma, beta, eps):
    return types.SimpleNamespace(weight=gamma, bias=beta, eps=eps)


class Kernels:
    """the runner of tests/rowwise_ref.py on the device, through the public wrappers"""

    def dev(self, t):
        return t.to(DEV)

    def host(self, t):
        torch.cuda.synchronize()
        return t.cpu()

    def add_ln(self, s, out=None, split_out=None):
        res = fused.add_ln(s["a"], _norm(s["gamma"], s["beta"], s["eps"]), residual=s["res"], bias=s["bias0"], relu=s["relu"],
                           num_partials=s["P"], post=s["post"], out=out, split=split_out is not None, a_scale=s["scale"],
                           split_lines=s["split"] == "lines", split_out=split_out)
        return res[0] if split_out is not None else res

    def rowgemm(self, gemms, rows):
        descs = []
        for gm in gemms:
            segs = [fused.row_seg(s["a"], num_partials=s["P"], a_scale=s["scale"], bias0=s["bias0"], residual=s["res"],
                                  norm=_norm(s["gamma"], s["beta"], s["eps"]) if s["gamma"] is not None else None, relu=s["relu"],
                                  post=s["post"], x_out=s["x_out"], split_out=s["split_out"], split_lines=s["split"] == "lines")
                    for s in gm["segs"]]
            descs.append(fused.row_gemm(segs, gm["W"], gm["b"], gm["out"], relu_from=gm["relu_from"]))
        fused.rowgemm_launch(descs, rows)

    def pe_head(self, x3, Wt, b, gamma, beta, eps):
        return fused.pe_head(x3, types.SimpleNamespace(weight=Wt, bias=b), _norm(gamma, beta, eps))

    def refine(self, prop, delta, td):
        return fused.refine_fused(prop, delta, td, W.NUM_RAY)

    def box_prep(self, boxes):
        return fused.box_prep(boxes.contiguous(), W.PC)

    def layer_boundary(self, prop, delta, td, Wt, b, gamma, beta, eps, xy_out):
        return fused.layer_boundary_fused(prop, delta, td, W.NUM_RAY, W.PC, types.SimpleNamespace(weight=Wt, bias=b), _norm(gamma, beta, eps),
                                          xy_out=xy_out)

    def gru_gate(self, gates, h_prev, h_out, bias_map, h_out2):
        fused.gru_gate_fused(gates, h_prev, h_out, bias_map=bias_map, h_out2=h_out2)

    def upsample2x(self, x):
        return fused.upsample2x_fused(x)


RUN = Kernels()


@pytest.fixture(scope="module")
def log():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    lg = W.Log()
    yield lg
    torch.set_num_threads(n)
    worst = lg.worst()
    print("\nrow-wise forwards against float64, worst per kernel in units of 2^-24 (E_ref | kernel | kernel / allowed):")
    for k in sorted(worst):
        print(f"  {k:>16s}: {worst[k]['E_ref']:8.3f} | {worst[k]['kernel']:8.3f} | {worst[k]['worst_ratio']:.3f}")
    path = os.environ.get("RAC_ROWWISE_ERRORS")
    if lg.errors and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(unit="2**-24", ratio_allowed=W.RATIO, floor=1.0, worst=worst, errors=lg.errors), f, indent=1, sort_keys=True)


@pytest.mark.parametrize("name", list(W.ROWGEMM_CASES))
def test_rowgemm_case(log, name):
    c = W.rowgemm_build(name)
    if name in W.ROWGEMM_INSTANTIATION:
        got = W.rowgemm_instantiation(c["rows"], [gm["N"] for gm in c["gemms"]], len(c["gemms"][0]["segs"]))
        assert got == W.ROWGEMM_INSTANTIATION[name]
    W.check_rowgemm(log, name, c, RUN)


@pytest.mark.parametrize("name", list(W.ADD_LN_CASES))
def test_add_ln_case(log, name):
    s = W.add_ln_build(name)
    assert W.add_ln_kernel(s["dim"], s["P"]) == W.ADD_LN_CASES[name]["kernel"]
    W.check_add_ln(log, name, s, RUN)


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
    """NaN and +-inf deltas: pred has NaN exactly where float64 has, xy is compared as the head reads it (nan_to_num), the rows
    beside the poisoned ones (their table and position-encoder rows included) stay within the bound"""
    W.check_refine(log, "B2 Q37 T3 poisoned", W.refine_case(77, 2, 37, 3, poison=True), RUN, boundary)


@pytest.mark.parametrize("name", list(W.GRU_CASES))
def test_gru_gate_case(log, name):
    c = W.gru_case(name)
    assert W.grid_stride("gru_gate", c["items"]) == (name == "past the cap")
    W.check_gru(log, name, c, RUN)


@pytest.mark.parametrize("name", list(W.UPSAMPLE_CASES))
def test_upsample2x_case(log, name):
    c = W.upsample_case(name)
    assert W.grid_stride("upsample2x", c["items"]) == (name == "past the cap")
    W.check_upsample(log, name, c, RUN)
