"""The two-stage float64 criterion of tests/test_fused_fwd_f64_gpu.py without a GPU: every case of tests/fused_fwd_ref.py with
the float32 restatement standing in for the kernels.  What this shows here: the inputs meet the band cap (BAND_CAP of the camera
gates) and the band holds the float32 chain's own error of the gated quantities; every "the case holds ..." assertion; the
reference alone passes its own bounds (A > 0 where expected, E_ref finite); every negative control fails as required; the
launcher rules the GPU module restates (rows per workgroup, variant, list_holes) select what the cases are named for; the
magnitude mode of the forward helpers equals the plain mode on non-negative inputs."""
import pytest
import torch

import bev_sampling_ref as BR
import fused_fwd_ref as F
import sampling4d_core_ref as SR

RUN = F.Restated32()


@pytest.fixture(scope="module")
def log():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    yield F.Log()
    torch.set_num_threads(n)


# --------------------------------------------------------------------------------------------------------------- sampling4d
@pytest.mark.parametrize("name", list(F.S4D_CASES))
def test_sampling4d_case(log, name):
    c, compact = F.s4d_build(name)
    F.check_s4d(log, name, c, RUN, compact, imposed=name in F.S4D_IMPOSED, gate_error=True)


def test_sampling4d_launcher_rules_reach_what_the_cases_are_named_for():
    seen = set()
    for name, spec in F.S4D_CASES.items():
        _, B, Q, G, T, NP, D, N, L, _, bf16, compact = spec
        P = NP * D
        rows = F.s4d_rows(P, L, N)
        if name.split()[0] in F.S4D_ROWS:
            assert rows == F.S4D_ROWS[name.split()[0]]
        seen.add((L, bf16, F.s4d_compact(N, P, compact)))
        seen.add((L, bf16, F.s4d_compact(N, P, False)))
    assert seen == {(L, bf, cp) for L in (2, 4, 5) for bf in (False, True) for cp in (False, True)}           # 12 instantiations
    assert not F.s4d_compact(3, 128, True) and F.s4d_compact(3, 64, None) and not F.s4d_compact(6, 12, None)
    rows8 = sorted(spec[2] for n, spec in F.S4D_CASES.items() if n.startswith("rows8"))
    assert rows8 == [1, 8 - 1, 8 + 1, 2 * 8 + 3]
    slots = {spec[1] * spec[3] * spec[4] for spec in F.S4D_CASES.values()}
    assert {3, 9, 12, 16} <= slots and {spec[7] for spec in F.S4D_CASES.values()} == {1, 3, 6}
    assert F.S4D_CASES["S9 odd GT"][3] * F.S4D_CASES["S9 odd GT"][4] % 2 == 1


def test_sampling4d_plain_slot_order_fails_stage_a(log):
    """quirk Q1 on an odd G*T: level weights read at (g, t) instead of t*G + g"""
    c, compact = F.s4d_build("S9 odd GT")
    table = RUN.table(c["query_bbox"])
    _, loc, w = RUN.s4d(c, table, None, compact)
    got, bound = F.s4d_stage_a(log, "S9 odd GT", c, table, loc, w, plain_slots=True)
    assert got > bound


def test_sampling4d_rows_beside_a_poisoned_query(log):
    c, compact = F.s4d_build("L4 f32 3cam")
    F.s4d_poison(c, 4)
    table = RUN.table(c["query_bbox"])
    out, loc, w = RUN.s4d(c, table, None, compact)
    check_rows_beside(log, "poisoned s4d", c, out, loc, w, 4)


def check_rows_beside(log, key, c, out, loc, w, q):
    keep = [i for i in range(c["Q"]) if i != q]
    assert bool(torch.isfinite(out[:, keep]).all()) and bool(torch.isfinite(loc[:, keep]).all()) and bool(torch.isfinite(w[:, keep]).all())
    cams = F.kernel_views(loc.nan_to_num(0.0), c["N"])
    ref, A, r32 = (F.s4d_gather(c, loc, w, cams), F.s4d_gather(c, loc, w, cams, magnitude=True), F.s4d_gather(c, loc, w, cams, F.F32))
    log.elementwise(key + " B out", out[:, keep], ref[:, keep], A[:, keep], r32[:, keep])


# ---------------------------------------------------------------------------------------------------------------------- BEV
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("name", list(F.BEV_SHAPES))
def test_bev_case(log, name, B, bf16):
    c = F.bev_build(name, B, bf16)
    assert F.bev_list_holes(c["T"], c["P"]) == F.BEV_HOLES[name]
    F.check_bev(log, f"{name} B{B} {'bf16' if bf16 else 'f32'}", c, RUN)


def test_bev_cases_reach_what_they_are_named_for():
    shapes = F.BEV_SHAPES.values()
    assert {s[3] for s in shapes} == {1, 3, 4} and {s[5] for s in shapes} >= {1, 5, 16}
    assert any(s[2] * s[3] % 4 for s in shapes) and {(s[6], s[7]) for s in shapes} == {(5, 7), (1, 9), (16, 16)}
    assert set(F.BEV_HOLES.values()) == {False, True}
    assert {s[4] * s[5] for s in shapes} >= {1, 6, 20, 32}
    # int16 lists: T*P a multiple of 8 (160) and not (18)
    assert not F.bev_list_holes(8, 20, i16=True) and F.bev_list_holes(3, 6, i16=True)


@pytest.mark.parametrize("name,B,bf16", [("P20 T8 h4 16x16", 1, False), ("P6 T3 h3 5x7", 2, True)])
def test_bev_two_streams(log, name, B, bf16):
    c = F.bev_build(name, B, bf16)
    cs = [c, F.bev_second_stream(c, 900)]
    assert not torch.equal(cs[0]["value"], cs[1]["value"]) and not torch.equal(cs[0]["sc"], cs[1]["sc"])
    table = RUN.table(c["query_bbox"])
    outs = RUN.bev_multi(cs, table)
    for i, (ci, o) in enumerate(zip(cs, outs)):
        single, loc = RUN.bev(ci, table)
        assert torch.equal(o, single)
        F.bev_stage_b(log, f"{name} B{B} stream {i}", ci, o, loc)


@pytest.mark.parametrize("name,B", [("P20 T8 h4 16x16", 1), ("P6 T3 h3 5x7", 1), ("P6 T3 h3 5x7", 2)])
def test_bev_int16(log, name, B):
    check_int16(log, name, B, RUN)


def check_int16(log, name, B, runner):
    c = F.bev_build(name, B)
    F.bev_octaves(c, 7)
    cs = [c, F.bev_second_stream(c, 901, octaves=True)]
    table = runner.table(c["query_bbox"])
    outs, qs, scales = runner.bev_q16(cs, table)
    for i, (ci, o, q, s) in enumerate(zip(cs, outs, qs, scales)):
        live = torch.log2(s[(q != 0).any(-1)])
        assert bool((q[0, :2] == 0).all()) and int(live.max() - live.min()) >= 16              # an all-zero block, many octaves
        _, loc = runner.bev(ci, table)                 # the float32 instantiation's locations: the same device chain
        value = q.double() * s.double()[..., None]
        key = f"{name} B{B} int16 stream {i}"
        _, A, bound = F.bev_stage_b(log, key, ci, o, loc, value=value)
        shifted = q.double() * torch.roll(s.double().flatten(), 1).reshape(s.shape)[..., None]
        F.must_fail(key + ": scales shifted by a block", o, F.bev_gather(ci, loc, value=shifted), A, bound)


def test_bev_rows_beside_a_poisoned_query(log):
    c = F.bev_build("P6 T3 h3 5x7", 1)
    F.bev_poison(c, 1)
    table = RUN.table(c["query_bbox"])
    out, loc = RUN.bev(c, table)
    check_bev_rows_beside(log, "poisoned bev", c, out, loc, 1)


def check_bev_rows_beside(log, key, c, out, loc, q):
    keep = [i for i in range(c["Q"]) if i != q]
    assert bool(torch.isfinite(out[:, keep]).all()) and bool(torch.isfinite(loc[:, keep]).all())
    ref, A, r32 = F.bev_gather(c, loc), F.bev_gather(c, loc, magnitude=True), F.bev_gather(c, loc, F.F32)
    log.elementwise(key + " B out", out[:, keep], ref[:, keep], A[:, keep], r32[:, keep])


# ---------------------------------------------------------------------------------------------------------- the helpers
def test_box_table_restatement_float32_against_float64(log):
    c, _ = F.s4d_build("S12 B2")
    F.check_box_table(log, "S12 B2", c["query_bbox"], RUN)
    assert 0 < log.errors["S12 B2 box table"]["E_ref"] < 1e3


def test_magnitude_mode_is_the_plain_mode_on_non_negative_inputs():
    c, _ = F.s4d_build("L4 f32 3cam")
    c["feats"] = [f.abs() for f in c["feats"]]
    _, loc, w = RUN.s4d(c, RUN.table(c["query_bbox"]))
    cams = F.kernel_views(loc, c["N"])
    assert torch.equal(F.s4d_gather(c, loc, w, cams), F.s4d_gather(c, loc, w, cams, magnitude=True))
    signed, _ = F.s4d_build("L4 f32 3cam")
    plain, mag = F.s4d_gather(signed, loc, w, cams), F.s4d_gather(signed, loc, w, cams, magnitude=True)
    assert bool((mag >= plain.abs()).all()) and not torch.equal(mag, plain)
    u, v = (SR.from_slots(loc[..., i].double(), c["B"], c["T"], c["G"]) for i in (0, 1))
    view = SR.from_slots(cams, c["B"], c["T"], c["G"])
    f64 = [f.double() for f in c["feats"]]
    assert torch.equal(SR.sampled64(f64, u, v, view, True), SR.sampled64(f64, u, v, view, True, magnitude=True))
    b = F.bev_build("P6 T3 h3 5x7", 2)
    b["value"] = b["value"].abs()
    _, bloc = RUN.bev(b, RUN.table(b["query_bbox"]))
    assert torch.equal(F.bev_gather(b, bloc), F.bev_gather(b, bloc, magnitude=True))
    loc_r = bloc.double()[0]
    assert torch.equal(BR.sampled64(b["value"][:3].double(), loc_r, b["hw"], True), BR.sampled64(b["value"][:3].double(), loc_r, b["hw"], True, True))
