"""The checkers of tests/test_head_loss_edges_gpu.py, checked without a GPU (helpers in tests/head_loss_edges_ref.py): the float64
restatements reproduce the float64 records of tests/golden/head_loss_small.npz -- which ties them to the original project's own
loss -- and every generated assignment problem is solved by rac_lsap_host with a valid certificate and scipy's total."""
import numpy as np
import pytest
import torch

import head_loss_edges_ref as ER
import loss_ref as LR
from decoder_grad_ref import bound

EPS32 = float(torch.finfo(torch.float32).eps)
TIE = bound(0)            # another summation order of the same float64 formula: 1e-5 of the largest element


@pytest.fixture(scope="module")
def g(golden_dir):
    return LR.load(golden_dir)


def tied(what, got, want64):
    want64 = np.asarray(want64, dtype=np.float64)
    mask = np.isfinite(want64)
    got = np.asarray(got, dtype=np.float64).reshape(want64.shape)
    assert (~mask).sum() <= 4 and np.array_equal(np.isfinite(got), mask), f"{what}: not finite where the record is, or the reverse"
    fig = LR.rel_err(got, want64, mask)
    print(f"  {what}: rel err {fig:.3e} (bound {TIE:.0e})")
    assert fig <= TIE, f"{what}: {fig:.3e}"


@pytest.mark.parametrize("case", LR.CASES)
def test_cost_ref_reproduces_the_fixture(g, case):
    a = LR.ASSIGNER
    for l, b, _ in LR.problems(g, case):
        got = ER.cost_ref(g[f"{case}:all_cls_scores"][l, b], g[f"{case}:all_bbox_preds"][l, b], g[f"{case}:gt_boxes{b}"],
                          g[f"{case}:gt_labels{b}"], LR.CODE_WEIGHTS, a["cls_cost"]["weight"], a["reg_cost"]["weight"],
                          a["theta_cost"]["weight"])
        c64 = g[f"{case}:cost64:{l}:{b}"].T
        tied(f"{case} cost_ref ({l},{b})", got.numpy(), c64)
        pinned = np.abs(c64) == 100.0
        assert np.array_equal(got.numpy()[pinned], c64[pinned])


def scaled(sums, grads, weight, avg):
    """the head's loss_weight / (avg_factor + eps) and nan_to_num on raw sums [L] and their unit gradients [L,...]"""
    factor = weight / (avg + EPS32)
    loss = torch.nan_to_num(sums * factor)
    keep = torch.isfinite(sums).double() * factor                  # (nan_to_num passes no gradient where it replaced)
    return loss, grads * keep.view(-1, *[1] * (grads.dim() - 1))


def check_losses(g, case, lc, lb, suffix):
    for l in range(LR.L):
        pre = "" if l == LR.L - 1 else f"d{l}."
        tied(f"{case} {pre}loss_cls{suffix}", lc[l].numpy(), g[f"{case}:loss64:{pre}loss_cls{suffix}"])
        tied(f"{case} {pre}loss_bbox{suffix}", lb[l].numpy(), g[f"{case}:loss64:{pre}loss_bbox{suffix}"])


@pytest.mark.parametrize("case", LR.CASES)
def test_det_loss_ref_reproduces_the_fixture_on_the_matching_rows(g, case):
    counts, Q = LR.counts_of(g, case), int(g[f"{case}:Q"])
    off = np.concatenate([[0], np.cumsum(counts)])
    target = np.full((LR.L, len(counts), Q), -1, np.int64)
    for l, b, _ in LR.problems(g, case):
        target[l, b, g[f"{case}:rows:{l}:{b}"]] = off[b] + g[f"{case}:cols:{l}:{b}"]
    gt = np.concatenate([g[f"{case}:gt_boxes{b}"] for b in range(len(counts))])
    labels = np.concatenate([g[f"{case}:gt_labels{b}"] for b in range(len(counts))])
    R = len(counts) * Q
    cls, box = g[f"{case}:all_cls_scores"], g[f"{case}:all_bbox_preds"]
    sums, gl, gb = ER.det_loss_ref(cls.reshape(LR.L, R, -1), box.reshape(LR.L, R, 10), target.reshape(LR.L, R), gt, labels, LR.CODE_WEIGHTS,
                                   LR.LOSS_CLS["alpha"], LR.LOSS_CLS["gamma"])
    n_pos = max(sum(min(Q, n) for n in counts), 1)
    lc, gl = scaled(sums[:, 0], gl, LR.LOSS_CLS["loss_weight"], n_pos)
    lb, gb = scaled(sums[:, 1], gb, LR.LOSS_BBOX["loss_weight"], n_pos)
    check_losses(g, case, lc, lb, "")
    tied(f"{case} grad all_cls_scores", gl.numpy(), g[f"{case}:grad64:all_cls_scores"])
    tied(f"{case} grad all_bbox_preds", gb.numpy(), g[f"{case}:grad64:all_bbox_preds"])


@pytest.mark.parametrize("case", LR.CASES)
def test_det_loss_ref_reproduces_the_fixture_on_the_denoising_rows(g, case):
    head = LR.loss_head(int(g[f"{case}:Q"]), dtype=torch.float64)
    _, _, preds, lv = LR.case_inputs(g, case, dtype=torch.float64)
    md = preds["dn_mask_dict"]
    known_labels, known_bboxs, dn_cls, dn_box, num_tgt = head.prepare_for_dn_loss(md)        # pure indexing
    total = int(md["batch_idx"].numel())
    sums, gl, gb = ER.det_loss_ref(dn_cls, dn_box, None, known_bboxs[:total], known_labels[:total], LR.CODE_WEIGHTS,
                                   LR.LOSS_CLS["alpha"], LR.LOSS_CLS["gamma"])
    lc, gl = scaled(sums[:, 0], gl, LR.LOSS_CLS["loss_weight"], max(num_tgt, 1))
    lb, gb = scaled(sums[:, 1], gb, LR.LOSS_BBOX["loss_weight"], max(num_tgt, 1))
    check_losses(g, case, head.dn_weight * lc, head.dn_weight * lb, "_dn")
    dn_cls.backward(head.dn_weight * gl)                                                    # back through the indexing to the leaves
    dn_box.backward(head.dn_weight * gb)
    tied(f"{case} grad dn_cls", lv["dn_cls"].grad.numpy(), g[f"{case}:grad64:dn_cls"])
    tied(f"{case} grad dn_box", lv["dn_box"].grad.numpy(), g[f"{case}:grad64:dn_box"])


@pytest.mark.parametrize("counts,Q,kind", ER.ASSIGN_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_generated_problems_have_certified_host_solutions(counts, Q, kind):
    scipy_opt = pytest.importorskip("scipy.optimize")
    problems, host = ER.launch_problems(kind, counts, Q), ER.host_solutions(kind, counts, Q)
    assert len(problems) == ER.L * len(counts)
    assert not any(torch.equal(problems[(0, b)][0], problems[(1, b)][0]) for b, G in enumerate(counts) if G * Q >= 25), "a matrix per layer"
    for (l, b), (cost, pi) in problems.items():
        G = counts[b]
        assert tuple(cost.shape) == (G, Q) and cost.dtype == torch.float32
        if G == 0:
            continue
        mq, mg, u, v, steps = host[(l, b)]
        LR.check_matching(mq, G, Q)
        total = LR.check_certificate(cost, mq, u, v)
        c64 = cost.double().numpy()
        r, c = scipy_opt.linear_sum_assignment(c64)
        want = float(c64[r, c].sum())
        assert abs(total - want) <= 1e-9 * max(1.0, abs(want)), (kind, l, b, total, want)
        assert G <= steps <= G * (G + 1) // 2
        if kind == "dominant":
            assert np.array_equal(r, np.arange(G)) and np.array_equal(c, pi), "scipy returns the planted matching"
            assert np.array_equal(mq.numpy(), pi) and steps == G and bool((v == 0).all())


def test_layout_builder():
    mats = {(l, b): torch.full((G, 5), float(10 * l + b)) for l in range(2) for b, G in enumerate((3, 0, 2))}
    out = ER.lay_out(mats, (3, 0, 2), 5, -7.0)
    assert tuple(out.shape) == (6, 3, 64)
    inside = torch.zeros_like(out, dtype=torch.bool)
    for (l, b), m in mats.items():
        assert torch.equal(out[l * 3 + b, :m.shape[0], :5], m)
        inside[l * 3 + b, :m.shape[0], :5] = True
    assert bool((out[~inside] == -7.0).all()) and int(inside.sum()) == 2 * 5 * 5
    assert bool(torch.isnan(ER.lay_out(mats, (3, 0, 2), 5, ER.NAN)[~inside]).all())


@pytest.mark.parametrize("C", [10, 3])
def test_match_cost_edges_are_where_they_were_planted(C):
    d = ER.match_cost_inputs(C)
    off = d["off"]
    for polar in (True, False):
        refs = ER.match_cost_refs(C, polar)
        assert sorted(refs) == [(l, b) for l in range(ER.L) for b in (0, 1, 3)]
        for (l, b), (c32, c64) in refs.items():
            assert tuple(c64.shape) == (ER.MC_COUNTS[b], ER.MC_Q) and bool(torch.isfinite(c64).all()) and bool(torch.isfinite(c32).all())
            want = torch.zeros_like(c64, dtype=torch.bool)
            if b == ER.MC_W0_BOX[0]:
                want[ER.MC_W0_BOX[1]] = True
            if b == ER.MC_BAD_LABEL[0]:
                want[ER.MC_BAD_LABEL[1]] = True
            if (l, b) == ER.MC_NAN_LOGIT[:2]:
                k = d["labels"][off[b] + 258]
                want[d["labels"][off[b]:off[b + 1]] == k, ER.MC_NAN_LOGIT[2]] = True
            assert torch.equal(c64 == 100.0, want) and torch.equal(c32 == 100.0, want) and not bool((c64 == -100.0).any())
    l, b, q = ER.MC_INF_LOGIT
    c32, c64 = ER.match_cost_refs(C, True)[(l, b)]
    assert bool(torch.isinf(d["cls"][l, b, q]).any()) and abs(float(c32[256, q]) - float(c64[256, q])) < 1e-4, "the +inf logit: a finite cost"
    for l, b, q in ER.MC_WRAP:
        xy = d["box"][l, b, q:q + 1, :2] * 2.0
        t32, t64 = float(ER.theta_turns(xy)), float(ER.theta_turns(xy.double()))
        assert t32 == 0.0 and 1.0 - 1e-7 < t64 < 1.0, "float32 wraps the angle to 0, float64 keeps it a hair below a full turn"
        c32, c64 = ER.match_cost_refs(C, True)[(l, b)]
        assert float((c32[:, q] - c64[:, q]).abs().max()) < 1e-4, "the circular distance agrees all the same"


@pytest.mark.parametrize("R,C", ER.DL_SHAPES)
@pytest.mark.parametrize("mode", ER.DL_TARGETS)
@pytest.mark.parametrize("alpha,gamma", ER.DL_FOCAL)
def test_det_loss_ref_is_finite_in_float32_on_the_extreme_logits(R, C, mode, alpha, gamma):
    d = ER.det_loss_inputs(R, C, mode)
    r32, r64 = ER.det_loss_refs(R, C, mode, alpha, gamma)
    assert all(bool(torch.isfinite(t).all()) for t in r64), "nothing non-finite is planted in these inputs"
    assert all(bool(torch.isfinite(t).all()) for t in r32), "float32 is finite wherever float64 is"
    assert all(t.dtype == torch.float32 for t in r32) and all(t.dtype == torch.float64 for t in r64)
    if R >= 1024:
        # (no box: no label position; one class and every row positive: no other position)
        want = (0 if mode.startswith("empty") else 6, 0 if (C == 1 and mode == "modulo") else 6)
        assert d["planted"] == want, "+-30, +-88, +-104 on label and other positions"
        for v in ER.DL_PLANTED:
            assert int((d["logits"] == v).sum()) == sum(want) // 6
    sums, gl, gb = r64
    if mode.startswith("empty"):
        assert bool((sums[:, 1] == 0).all()) and bool((gb == 0).all()) and bool((sums[:, 0] > 0).all())
    else:
        assert len(d["h0_rows"]) >= (ER.L if R > 1 else 0) and all(bool((gb[l, r] == 0).all()) for l, r in d["h0_rows"])
        assert len(d["exact_rows"]) >= 1
        for l, r in d["exact_rows"]:
            assert bool((gb[l, r, ER.DL_PASS_THROUGH] == 0).all()) and bool((gb[l, r, [2, 3, 5, 6, 7]] != 0).all())
        if R > 1024:
            assert any(r >= 1024 for _, r in d["exact_rows"]), "a planted row in the second trip of the row loop"
    # the textbook gradient of the box term: the sign of the difference times the code weight
    assert set(np.unique(gb.numpy()).tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
