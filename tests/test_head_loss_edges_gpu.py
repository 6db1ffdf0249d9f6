"""rac_match_cost_fwd, rac_lsap_fwd and rac_det_loss_fwd on the MI355X past the shapes of tests/golden/head_loss_small.npz, against
the float64 restatements and generated problems of tests/head_loss_edges_ref.py (checked without a GPU by
tests/test_head_loss_edges_cpu.py).  What each shape is for:

  match cost   Q = 300: a second, ragged block of 256 queries; 300 and 257 boxes: a second staging trip of the ground truth with a
               44-box and a 1-box tail; an empty sample; C = 3 besides 10; HungarianAssigner3D (no theta) besides the polar one;
               a label out of range, a w = 0 box, a NaN and a +inf logit, an angle that float32 wraps to 0 and float64 does not
  assignment   Q < 64, Q = 64, 65, square problems, Q = 900 (15 queries a lane), Q = 2048 (32 a lane), G = Q = 2048 (the full LDS
               carve, 63488 bytes), four samples of different sizes a launch, ties, +-100 pins, duplicate rows, the give-up path
  det loss     R = 1100 and 1024 (a second trip of the 1024-thread row loop, ragged and not), R = 1, C = 1, gamma = 1.5 (powf),
               alpha = 0.4, no ground truth at all, logits up to +-104

Costs, sums and gradients follow loss_ref.assert_close's rule: max-normalised error against float64 within bound(e32), e32 the
restatement's own float32-against-float64 figure."""
import time

import numpy as np
import pytest
import torch

import head_loss_edges_ref as ER
import loss_ref as LR
from racformer_amd import fused
from racformer_amd.fused import det_loss_fused, lsap_fused, match_cost_fused
from racformer_amd.head import RaCFormer_head
from racformer_amd.losses import head_loss_sums

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
IDS = dict(ids=lambda v: str(v).replace(" ", ""))


# ------------------------------------------------------------------------------------------------ match cost
@pytest.mark.parametrize("polar", [True, False])
@pytest.mark.parametrize("C", [10, 3])
def test_match_cost_second_block_second_staging_trip(C, polar):
    d, refs, a = ER.match_cost_inputs(C), ER.match_cost_refs(C, polar), LR.ASSIGNER
    counts, Q, B, off = list(ER.MC_COUNTS), ER.MC_Q, ER.MC_B, d["off"]
    cls, box, gt, labels = (d[k].to(DEV) for k in ("cls", "box", "gt", "labels"))
    cw = torch.tensor(LR.CODE_WEIGHTS, device=DEV)
    keep = [t.clone() for t in (cls, box, gt, labels, cw)]
    outs = []
    for fill in (NAN, -1e30):
        out = torch.full((ER.L * B, max(counts), (Q + 63) // 64 * 64), fill, device=DEV)
        match_cost_fused(cls, box, gt, labels, counts, cw, a["cls_cost"]["weight"], a["reg_cost"]["weight"],
                         a["theta_cost"]["weight"] if polar else None, out=out)
        outs.append(out.cpu())
    assert all(torch.equal(x.nan_to_num(7.0), y.nan_to_num(7.0)) for x, y in zip((cls, box, gt, labels, cw), keep)), "the kernel wrote its inputs"
    written = torch.zeros_like(outs[0], dtype=torch.bool)
    for (l, b), (c32, c64) in refs.items():
        p = l * B + b
        got = outs[0][p, :counts[b], :Q]
        written[p, :counts[b], :Q] = True
        pinned = c64.abs() == 100.0
        ER.figures(f"C={C} polar={polar} cost ({l},{b})", got, c32, c64, mask=~pinned.numpy())
        assert torch.equal(got[pinned], c64[pinned].float()), "NaN / inf entries must land exactly on +-100"
        if b == ER.MC_BAD_LABEL[0]:
            assert bool((got[ER.MC_BAD_LABEL[1]] == 100.0).all()), "a label outside the classes: 100 throughout"
        if b == ER.MC_W0_BOX[0]:
            assert bool((got[ER.MC_W0_BOX[1]] == 100.0).all()), "the w = 0 box: 100 throughout"
    # nothing outside g < G_b, q < Q is written, and what is written does not depend on what was there
    assert int(written.sum()) == ER.L * sum(counts) * Q
    assert bool(torch.isnan(outs[0][~written]).all()) and bool((outs[1][~written] == -1e30).all())
    assert torch.equal(outs[0][written], outs[1][written])


# ------------------------------------------------------------------------------------------------ assignment
def check_problem(what, cost, G, Q, offset, matched, assigned, u, v, steps, host_total, pi=None):
    """one problem's outputs (CPU tensors, this problem's rows) against the certificate and the host solver's total"""
    if G == 0:
        assert bool((assigned == -1).all()) and bool((matched == -1).all()) and int(steps) == 0, f"{what}: no box, all background"
        return
    LR.check_matching(matched, G, Q)
    assert bool((matched[G:] == -1).all()) and bool((u[G:] == 0).all()), f"{what}: beyond the sample's boxes"
    total = LR.check_certificate(cost, matched, u, v)
    assert abs(total - host_total) <= 1e-9 * max(1.0, abs(host_total)), f"{what}: total {total!r}, rac_lsap_host {host_total!r}"
    back = torch.full((Q,), -1, dtype=torch.int32)
    back[matched[:G].long()] = torch.arange(G, dtype=torch.int32) + offset
    assert torch.equal(assigned, back), f"{what}: assigned_gt is the inverse of matched_query, offset into the table"
    assert G <= int(steps) <= G * (G + 1) // 2, f"{what}: {int(steps)} steps"
    if pi is not None:
        assert int(steps) == G and np.array_equal(matched[:G].numpy(), pi), f"{what}: every augmentation ends in one step, at the planted query"


@pytest.mark.parametrize("counts,Q,kind", ER.ASSIGN_CASES, **IDS)
def test_lsap_on_generated_problems(counts, Q, kind):
    problems, host = ER.launch_problems(kind, counts, Q), ER.host_solutions(kind, counts, Q)
    B, off = len(counts), np.concatenate([[0], np.cumsum(counts)])
    runs, wall = [], []
    for fill in (NAN, NAN, -1e30):
        cost = ER.lay_out(problems, counts, Q, fill).to(DEV)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        runs.append(lsap_fused(cost, list(counts), ER.L, Q, with_steps=True))
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
    for other in runs[1:]:                  # two runs: the same bits; the pad entries never influence a result
        assert all(torch.equal(x, y) for x, y in zip(runs[0], other))
    matched, assigned, u, v, steps = (t.cpu() for t in runs[0])
    assert matched.dtype == assigned.dtype == steps.dtype == torch.int32 and u.dtype == v.dtype == torch.float64
    assert tuple(matched.shape) == (ER.L * B, max(counts)) and tuple(assigned.shape) == (ER.L * B, Q)
    print(f"  {kind} {counts} Q={Q}: Dijkstra steps per problem {steps.tolist()}, launch {min(wall) * 1e3:.2f} ms")
    for (l, b), (c, pi) in problems.items():
        p = l * B + b
        check_problem(f"{kind} ({l},{b})", c, counts[b], Q, int(off[b]), matched[p], assigned[p], u[p], v[p], steps[p],
                      ER.total_of(c, host[(l, b)][0]) if counts[b] else 0.0, pi)


@pytest.mark.parametrize("bad", [float("inf"), NAN], ids=["inf_row", "nan_row"])
def test_lsap_gives_a_problem_up_and_leaves_its_neighbours_alone(bad):
    """a row without a finite entry has no assignment: the kernel's ordinary return for it is 'unmatched throughout' with a negative
    step count, and the problems before and after it in the launch come out as if it were solvable"""
    counts, Q = (9, 12, 70), 70
    rng = np.random.default_rng(77)
    mats = {(0, b): torch.from_numpy(rng.normal(size=(G, Q)).astype(np.float32)) for b, G in enumerate(counts)}
    broken = dict(mats)
    broken[(0, 1)] = mats[(0, 1)].clone()
    broken[(0, 1)][5] = bad
    fine = lsap_fused(ER.lay_out(mats, counts, Q, NAN, num_layers=1).to(DEV), list(counts), 1, Q, with_steps=True)
    got = lsap_fused(ER.lay_out(broken, counts, Q, NAN, num_layers=1).to(DEV), list(counts), 1, Q, with_steps=True)
    fine, got = [t.cpu() for t in fine], [t.cpu() for t in got]
    matched, assigned, u, v, steps = got
    assert bool((matched[1] == -1).all()) and bool((assigned[1] == -1).all()) and bool((u[1] == 0).all()) and bool((v[1] == 0).all())
    assert int(steps[1]) < 0
    for p in (0, 2):
        assert all(torch.equal(x[p], y[p]) for x, y in zip(fine, got)), "the neighbours of the problem given up"
    off = [0, 9, 21]
    for p, G in enumerate(counts):          # and the launch they are compared with is itself right
        check_problem(f"finite ({p})", mats[(0, p)], G, Q, off[p], *(t[p] for t in fine), ER.total_of(mats[(0, p)], fused.lsap_host(cost_gq=mats[(0, p)])[0]))


# ------------------------------------------------------------------------------------------------ what the wrappers refuse
def test_wrappers_refuse_what_the_kernels_do_not_take(monkeypatch):
    with pytest.raises(RuntimeError, match="larger problems take rac_lsap_host"):
        lsap_fused(torch.zeros(2, 1, 2112, device=DEV), [1], 2, 2049)
    with pytest.raises(RuntimeError, match="larger problems take rac_lsap_host"):
        lsap_fused(torch.zeros(2, 5, 64, device=DEV), [5], 2, 4)
    with pytest.raises(RuntimeError, match="at most 64 samples"):
        lsap_fused(torch.zeros(65, 1, 64, device=DEV), [1] * 65, 1, 4)
    with pytest.raises(RuntimeError, match="at most 64 samples"):
        match_cost_fused(torch.zeros(1, 65, 4, 10, device=DEV), torch.zeros(1, 65, 4, 10, device=DEV), torch.ones(65, 9, device=DEV),
                         torch.zeros(65, dtype=torch.int32, device=DEV), [1] * 65, torch.ones(10, device=DEV), 2.0, 0.25, 3.0)
    # more boxes than queries: RaCFormer_head.loss takes loss_unfused (the host solver), not the device solver
    Q, G = 4, 6
    head = RaCFormer_head(num_classes=LR.NUM_CLASSES, in_channels=LR.EMBED, num_query=Q, num_clusters=2, code_size=10,       # (two rays of two)
                          code_weights=LR.CODE_WEIGHTS, query_denoising=False, sync_cls_avg_factor=True, transformer=None,
                          bbox_coder=dict(type="NMSFreeCoder", post_center_range=LR.POST_RANGE, pc_range=LR.PC_RANGE, max_num=Q,
                                          score_threshold=0.05, num_classes=LR.NUM_CLASSES),
                          loss_cls=LR.LOSS_CLS, loss_bbox=LR.LOSS_BBOX, loss_iou=LR.LOSS_IOU, train_cfg=dict(assigner=LR.ASSIGNER)).to(DEV).train()
    rng = np.random.default_rng(4)
    gt, lab = ER.gt_table(rng, G, LR.NUM_CLASSES)
    preds = {"all_cls_scores": torch.from_numpy(rng.normal(-2.0, 1.5, (ER.L, 1, Q, LR.NUM_CLASSES)).astype(np.float32)).to(DEV),
             "all_bbox_preds": torch.from_numpy(ER.pred_boxes(rng, (ER.L, 1, Q))).to(DEV), "enc_cls_scores": None, "enc_bbox_preds": None,
             "dn_mask_dict": None}
    gts, labels = [torch.from_numpy(gt).to(DEV)], [torch.from_numpy(lab).long().to(DEV)]

    def no_launch(*a, **k):
        raise AssertionError("the fused route was taken")
    monkeypatch.setattr(fused, "lsap_fused", no_launch)
    monkeypatch.setattr(fused, "match_cost_fused", no_launch)
    out, want = head.loss(gts, labels, preds), head.loss_unfused(gts, labels, preds)
    assert sorted(out) == sorted(want) and len(out) == 2 * ER.L
    assert all(torch.equal(out[k], want[k]) and bool(torch.isfinite(out[k]).all()) for k in want)


# ------------------------------------------------------------------------------------------------ detection loss
@pytest.mark.parametrize("alpha,gamma", ER.DL_FOCAL, **IDS)
@pytest.mark.parametrize("mode", ER.DL_TARGETS)
@pytest.mark.parametrize("R,C", ER.DL_SHAPES, **IDS)
def test_det_loss_second_row_trip_powf_and_extreme_logits(R, C, mode, alpha, gamma):
    d = ER.det_loss_inputs(R, C, mode)
    r32, r64 = ER.det_loss_refs(R, C, mode, alpha, gamma)
    assert all(bool(torch.isfinite(t).all()) for t in r64), "no non-finite reference entry is planted: none may be left out"
    logits, boxes, gt, labels = (d[k].to(DEV) for k in ("logits", "boxes", "gt", "labels"))
    target = d["target"].to(DEV) if d["target"] is not None else None
    cw = torch.tensor(LR.CODE_WEIGHTS, device=DEV)
    keep = [t.clone() for t in (logits, boxes, gt)]
    a = det_loss_fused(logits, boxes, target, gt, labels, cw, alpha, gamma)
    b = det_loss_fused(logits, boxes, target, gt, labels, cw, alpha, gamma)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "two runs: the same bits"
    assert all(torch.equal(x, y) for x, y in zip((logits, boxes, gt), keep)), "the kernel wrote its inputs"
    sums, gl, gb = (t.cpu() for t in a)
    what = f"R={R} C={C} {mode} alpha={alpha} gamma={gamma}"
    assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(gl).all()) and bool(torch.isfinite(gb).all())
    ER.figures(f"{what} sum cls", sums[:, 0], r32[0][:, 0], r64[0][:, 0])
    ER.figures(f"{what} sum box", sums[:, 1], r32[0][:, 1], r64[0][:, 1])
    ER.figures(f"{what} grad_logits", gl, r32[1], r64[1])
    ER.figures(f"{what} grad_boxes", gb, r32[2], r64[2])
    if mode.startswith("empty"):
        assert bool((sums[:, 1] == 0).all()) and bool((gb == 0).all()), "no ground truth: pure background, box gradients exactly 0"
    else:
        tgt = d["target"] if d["target"] is not None else (torch.arange(R) % gt.shape[0]).expand(ER.L, R)
        assert bool((gb[tgt < 0] == 0).all()), "background rows carry zero box gradient"
        for l, r in d["h0_rows"]:
            assert bool((gb[l, r] == 0).all()), "the row with the non-finite target has no box gradient"
        for l, r in d["exact_rows"]:
            assert bool((gb[l, r, ER.DL_PASS_THROUGH] == 0).all()), "a coordinate equal to its target: gradient exactly 0"
    # through autograd with another upstream gradient per layer and sum
    up = torch.tensor([[0.5, 2.0], [-3.0, 0.25]], device=DEV)
    x, bx = logits.clone().requires_grad_(), boxes.clone().requires_grad_()
    out = head_loss_sums(x, bx, target, gt, labels, cw, alpha, gamma)
    assert torch.equal(out.detach(), a[0])
    out.backward(up)
    scale = up.cpu().double()
    for name, grad, k, col in (("logits", x.grad, 1, 0), ("boxes", bx.grad, 2, 1)):
        s = scale[:, col].view(-1, 1, 1)
        ER.figures(f"{what} backward {name}", grad.cpu(), r32[k] * s.float(), r64[k] * s)
