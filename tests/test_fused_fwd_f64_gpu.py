"""rac_sampling4d_fwd and the rac_bev_sampling_*fwd family on the MI355X against float64, stage by stage (tests/fused_fwd_ref.py
holds the cases, references, bounds and negative controls; tests/test_fused_fwd_f64_cpu.py runs the same checks on the CPU with the
float32 restatement in the kernels' place).

Stage A: the kernels' own keypoints (``debug=True``: loc_out, w_out) against the float64 chain on the same float32 inputs and the
device's own box table, point by point; cameras equal to float64's outside a band of 1e-4 around the discrete gates (at most 2 %
of a case's points, asserted on the CPU from float64 alone) and among the cameras float64 allows inside it.
Stage B: EVERY element of ``out`` against the float64 gather at the kernel's own locations, cameras and (sampling4d) level weights:
|got - ref| <= max(4 x E_ref, 1) x 2^-24 x A, A the same sum with every term non-negative, E_ref the float32 restatement's own worst
err / A on the same case; an element with A == 0 is exactly 0.  Every comparison prints its (E_ref, kernel) pair; with
RAC_FUSED_FWD_ERRORS=<file> the session's pairs are written there as JSON (profiles/fused_fwd_f64.json is the MI355X run's copy).

Reached, and asserted as reached through the launchers' rules restated in tests/fused_fwd_ref.py: the 12 instantiations of
rac_sampling4d_fwd ({f32, bf16} x L in {2, 4, 5} x {plain, COMPACT}; COMPACT and plain bitwise equal on the 3-camera rig), 8 / 4 / 2
query rows per workgroup with ragged last workgroups (Q = 1, rows - 1, rows + 1, 2 * rows + 3), P = 128 with COMPACT asked (plain
taken), S = 3 / 9 / 12 / 16 slots (B = 2, odd G*T), N = 1 / 3 / 6 cameras, imposed cameras, strided Linear outputs; the three BEV
instantiations, list_holes 0 and 1, B = 2 (its LDS layout and frame / batch pairing), Q * heads not a multiple of 4, two streams
(bitwise the single-stream launches), int16 block storage; a query poisoned with NaN / inf beside clean ones.
Negative controls, each failing its check: one tap dropped (every stage B comparison), level weights in plain slot order on an odd
G*T, the frame / batch pairing undone at B = 2, the int16 scale table shifted by one block.

Measured on the MI355X, worst over the session in units of 2^-24 (E_ref | kernel):
  sampling4d  stage B out 3.80 | 5.24    stage A level weights 2.17 | 2.17    box table 420 | 433
              stage A u 1921 | 3285, v 164 | 122 (case "rows4 Q11": its worst point has a small positive homo, which divides the
              float32 error of camx; the median case has 34 | 25 for u) -- never above 0.44 of what 4 x E_ref allows
  BEV         stage B out 6.15 | 6.58 (f32, bf16, int16, two streams)    stage A loc 10.0 | 13.1
Before this module the BEV forward formed its pixel coordinates with one fused multiply-add (hipcc contracted ``loc * W - 0.5``),
the backward and every reference with two roundings: stage B then measured up to 76 (1 x 9 map, P = 1, B = 2), 65 (1 x 9, P = 6)
and 49 (int16, 5 x 7) where 9.6, 15.4 and 19.9 were allowed -- a tap weight an ulp of the coordinate off shows in full in an element
whose heavier tap holds a value near 0.  bev_fused.hip now rounds the two operations separately (power-of-two maps: the same bits)."""
import json
import os

import pytest
import torch

import fused_fwd_ref as F
from racformer_amd.fused import (bev_sampling_fused, bev_sampling_multi_fused, box_prep, quantize_values_i16, sampling4d_fused)
from test_fused_fwd_f64_cpu import check_bev_rows_beside, check_int16, check_rows_beside

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Kernels:
    """the runner of tests/fused_fwd_ref.py on the device: CPU tensors in, CPU tensors out"""

    def table(self, query_bbox):
        return box_prep(query_bbox.to(DEV), F.PC).cpu()

    def s4d(self, c, table, view_in=None, compact=None):
        v = F.s4d_slice(c, c["wide"].to(DEV))
        assert all(x.stride(-2) > x.shape[-1] and x.stride(-1) == 1 for x in v.values())           # column slices of one wider tensor
        res = sampling4d_fused([f.to(DEV) for f in c["feats"]], c["query_bbox"].to(DEV), v["off"], v["ray"], v["sc"], c["td"].to(DEV),
                               c["l2i"].to(DEV), c["T"], c["G"], c["NP"], c["D"], F.PC, F.D_REGION, F.IMG[0], F.IMG[1], eps=F.EPS, debug=True,
                               box_table=table.to(DEV), view_in=None if view_in is None else view_in.to(DEV).contiguous(), compact=compact)
        torch.cuda.synchronize()
        return tuple(x.cpu() for x in res)

    @staticmethod
    def _bev_args(c, value=None):
        value = c["value"] if value is None else value
        return tuple(x.to(DEV) for x in (value, c["off"], c["ray"], c["sc"], c["qu"]))

    @staticmethod
    def _bev_cfg(c):
        return c["T"], c["heads"], c["NP"], c["D"], F.PC, F.D_REGION

    def bev(self, c, table, value=None):
        value, *lin = self._bev_args(c, value)
        out, loc = bev_sampling_fused(value, c["hw"], c["query_bbox"].to(DEV), *lin, c["time_diff"].to(DEV), *self._bev_cfg(c), debug=True,
                                      box_table=table.to(DEV))
        torch.cuda.synchronize()
        return out.cpu(), loc.cpu()

    def bev_multi(self, cs, table, quantize=False):
        c = cs[0]
        streams = [self._bev_args(ci) for ci in cs]
        scales = None
        if quantize:
            qs, scales = zip(*(quantize_values_i16(s[0]) for s in streams))
            streams = [(q,) + s[1:] for q, s in zip(qs, streams)]
        out = torch.full((len(cs), c["B"], c["Q"], c["heads"] * 64), float("nan"), device=DEV)
        bev_sampling_multi_fused(streams, c["hw"], c["query_bbox"].to(DEV), c["time_diff"].to(DEV), *self._bev_cfg(c), table.to(DEV), out,
                                 value_scales=None if scales is None else list(scales))
        torch.cuda.synchronize()
        outs = [o.cpu() for o in out]
        return (outs, [q.cpu() for q in qs], [s.cpu() for s in scales]) if quantize else outs

    def bev_q16(self, cs, table):
        return self.bev_multi(cs, table, quantize=True)


RUN = Kernels()


@pytest.fixture(scope="module")
def log():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    lg = F.Log()
    yield lg
    torch.set_num_threads(n)
    worst = {}
    for key, e in lg.errors.items():
        kind = ("bev " if key.startswith(("P", "poisoned bev")) else "sampling4d ") + " ".join(key.split()[-2:])
        w = worst.setdefault(kind, dict(E_ref=0.0, kernel=0.0, worst_ratio=0.0))
        w["E_ref"], w["kernel"] = max(w["E_ref"], e["E_ref"]), max(w["kernel"], e["kernel"])
        w["worst_ratio"] = max(w["worst_ratio"], e["kernel"] / F.bound_of(e["E_ref"]))
    print("\nfused forwards against float64, worst per kind in units of 2^-24 (E_ref | kernel | kernel / allowed):")
    for k in sorted(worst):
        print(f"  {k:>28s}: {worst[k]['E_ref']:8.3f} | {worst[k]['kernel']:8.3f} | {worst[k]['worst_ratio']:.3f}")
    path = os.environ.get("RAC_FUSED_FWD_ERRORS")
    if lg.errors and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(unit="2**-24", ratio_allowed=F.RATIO, floor=1.0, worst=worst, errors=lg.errors), f, indent=1, sort_keys=True)


# --------------------------------------------------------------------------------------------------------------- sampling4d
@pytest.mark.parametrize("name", list(F.S4D_CASES))
def test_sampling4d_case(log, name):
    c, compact = F.s4d_build(name)
    kind = name.split()[0]
    if kind in F.S4D_ROWS:
        assert F.s4d_rows(c["P"], c["L"], c["N"]) == F.S4D_ROWS[kind]
    if name.endswith("cam"):
        assert F.s4d_compact(c["N"], c["P"], compact)
    got = F.check_s4d(log, name, c, RUN, compact, imposed=name in F.S4D_IMPOSED)
    if name.endswith("3cam") or kind == "rows2":
        # the other variant on the same inputs, bit for bit (rows2: P = 128 takes the plain variant whatever is asked)
        assert F.s4d_compact(c["N"], c["P"], compact) == (kind != "rows2") and not F.s4d_compact(c["N"], c["P"], False)
        plain = RUN.s4d(c, RUN.table(c["query_bbox"]), None, False)
        assert all(torch.equal(a, b) for a, b in zip(got, plain))


def test_sampling4d_plain_slot_order_fails_stage_a(log):
    c, compact = F.s4d_build("S9 odd GT")
    table = RUN.table(c["query_bbox"])
    _, loc, w = RUN.s4d(c, table, None, compact)
    got, bound = F.s4d_stage_a(log, "S9 odd GT", c, table, loc, w, plain_slots=True)
    print(f"level weights against the plain slot order: {got:.3g} x 2^-24 (allowed {bound:.3g})")
    assert got > bound


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "plain"])
def test_sampling4d_rows_beside_a_poisoned_query(log, compact):
    """s4d_taps_of_level: a NaN / inf coordinate fails ``in`` before any offset is formed (every tap S4D_TAP_OUTSIDE)"""
    c, _ = F.s4d_build("L4 f32 3cam")
    F.s4d_poison(c, 4)
    table = RUN.table(c["query_bbox"])
    out, loc, w = RUN.s4d(c, table, None, compact)
    assert not bool(torch.isfinite(loc[:, 4]).all())
    check_rows_beside(log, f"poisoned sampling4d {'compact' if compact else 'plain'}", c, out, loc, w, 4)


# ---------------------------------------------------------------------------------------------------------------------- BEV
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", list(F.BEV_SHAPES))
def test_bev_case(log, name, B, bf16):
    c = F.bev_build(name, B, bf16)
    assert F.bev_list_holes(c["T"], c["P"]) == F.BEV_HOLES[name]
    F.check_bev(log, f"{name} B{B} {'bf16' if bf16 else 'f32'}", c, RUN)


def test_box_prep_against_float64(log):
    for name in ("S12 B2", "rows8 Q19"):
        c, _ = F.s4d_build(name)
        F.check_box_table(log, name, c["query_bbox"], RUN)


@pytest.mark.parametrize("name,B,bf16", [("P20 T8 h4 16x16", 1, False), ("P6 T3 h3 5x7", 2, True)])
def test_bev_two_streams(log, name, B, bf16):
    """each stream of the two-stream launch (grid dimension y) is the single-stream launch on its arguments bit for bit, so
    stage B carries over; checked on the streams' outputs all the same"""
    c = F.bev_build(name, B, bf16)
    cs = [c, F.bev_second_stream(c, 900)]
    table = RUN.table(c["query_bbox"])
    outs = RUN.bev_multi(cs, table)
    for i, (ci, o) in enumerate(zip(cs, outs)):
        single, loc = RUN.bev(ci, table)
        assert torch.equal(o, single)
        F.bev_stage_b(log, f"{name} B{B} stream {i}", ci, o, loc)
    assert not torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("name,B", [("P20 T8 h4 16x16", 1), ("P6 T3 h3 5x7", 1), ("P6 T3 h3 5x7", 2)])
def test_bev_int16(log, name, B):
    """the int16 instantiation (8 lanes per tap row) at the float32 instantiation's locations: the reference reads q * scale"""
    T, P = F.BEV_SHAPES[name][1], F.BEV_SHAPES[name][4] * F.BEV_SHAPES[name][5]
    assert F.bev_list_holes(T, P, i16=True) == (T * P % 8 != 0)
    check_int16(log, name, B, RUN)


@pytest.mark.parametrize("B", [1, 2])
def test_bev_rows_beside_a_poisoned_query(log, B):
    """bev_polar_jitter: fminf(fmaxf(x, 0), 1) turns a NaN location into 0 and +-inf into a bound before the footprint is formed"""
    c = F.bev_build("P6 T3 h3 5x7", B)
    F.bev_poison(c, 1)
    table = RUN.table(c["query_bbox"])
    out, loc = RUN.bev(c, table)
    check_bev_rows_beside(log, f"poisoned bev B{B}", c, out, loc, 1)
