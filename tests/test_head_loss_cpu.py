"""RaCFormer_head.loss without a GPU: the torch match costs, the host assignment solver (rac_lsap_host) and the head's CPU route
against the REFERENCE's own loss (tests/golden/head_loss_small.npz, helpers in tests/loss_ref.py).  All of these fail on a tree
without the losses: the classes do not exist there and ``loss`` raises."""
import numpy as np
import pytest
import torch

import loss_ref as LR
from racformer_amd import losses
from racformer_amd.fused import lsap_host


@pytest.fixture(scope="module")
def g(golden_dir):
    return LR.load(golden_dir)


def assigner_inputs(g, case, l, b):
    cls = torch.from_numpy(g[f"{case}:all_cls_scores"][l, b])
    box = torch.from_numpy(g[f"{case}:all_bbox_preds"][l, b])
    return box, cls, torch.from_numpy(g[f"{case}:gt_boxes{b}"]), torch.from_numpy(g[f"{case}:gt_labels{b}"])


@pytest.mark.parametrize("case", LR.CASES)
def test_cost_callables_reproduce_the_fixture(g, case):
    a = losses.build_assigner(LR.ASSIGNER)
    cw = torch.tensor(LR.CODE_WEIGHTS)
    for l, b, _ in LR.problems(g, case):
        box, cls, gt, lab = assigner_inputs(g, case, l, b)
        keep = (box.clone(), cls.clone(), gt.clone())
        cost = a.cost(box, cls, gt, lab, cw, True).numpy()
        assert all(torch.equal(x, y) or (torch.isnan(x) == torch.isnan(y)).all() for x, y in zip((box, cls, gt), keep)), "inputs were written"
        c32, c64 = g[f"{case}:cost32:{l}:{b}"], g[f"{case}:cost64:{l}:{b}"]
        LR.assert_close(f"{case} cost ({l},{b})", cost, c32, c64)
        pinned = np.abs(c64) == 100.0
        assert np.array_equal(cost[pinned], c64[pinned].astype(np.float32)), "NaN / inf entries must land exactly on +-100"
    if case == "c":
        assert (g["c:cost64:0:0"] == 100.0).any(), "the NaN logit is in the fixture"
    if case == "b":
        assert (g["b:cost64:0:1"] == 100.0).all(), "the w = 0 box has a constant row"


def test_single_costs_are_plain_torch_callables():
    gen = torch.Generator().manual_seed(0)
    pred, gt = torch.randn(7, 10, generator=gen), torch.randn(3, 10, generator=gen)
    assert torch.equal(losses.BBox3DL1Cost(0.25)(pred, gt), torch.cdist(pred, gt, p=1) * 0.25)
    # two centres on either side of the +x axis: the angles differ by almost a full turn, the wrapped cost is small
    a = torch.tensor([[10.0, -0.1] + [0.0] * 8])
    b = torch.tensor([[10.0, 0.1] + [0.0] * 8])
    t = losses.ThetaL1Cost(1.0)(a, b)
    assert 0 < float(t) < 0.01
    assert float(losses.ThetaL1Cost(3.0)(a, -a)) == pytest.approx(1.5, abs=1e-5)      # opposite rays: half a turn
    x = torch.randn(7, 10, generator=gen)
    lab = torch.tensor([1, 1, 4])
    p = x.sigmoid()
    want = (-(p + 1e-12).log() * 0.25 * (1 - p) ** 2 + (1 - p + 1e-12).log() * 0.75 * p ** 2)[:, lab] * 2.0
    assert torch.allclose(losses.FocalLossCost(2.0)(x, lab), want)


@pytest.mark.parametrize("case", LR.CASES)
def test_host_solver_on_the_fixture(g, case):
    scipy_opt = pytest.importorskip("scipy.optimize")
    Q = int(g[f"{case}:Q"])
    for l, b, margin in LR.problems(g, case):
        cost = torch.from_numpy(g[f"{case}:cost32:{l}:{b}"])                      # [Q,G], the reference's layout
        G = cost.shape[1]
        mq, mg, u, v, steps = lsap_host(cost_qg=cost)
        LR.check_matching(mq, G, Q)
        assert all(int(mg[int(q)]) == i for i, q in enumerate(mq)) and int((mg >= 0).sum()) == G
        total = LR.check_certificate(cost.t(), mq, u, v)
        r, c = scipy_opt.linear_sum_assignment(cost.double().numpy())
        want = float(cost.double().numpy()[r, c].sum())
        assert abs(total - want) <= 1e-9 * max(1.0, abs(want))
        assert abs(total - float(g[f"{case}:total64:{l}:{b}"])) <= 1e-9 * max(1.0, abs(want))
        assert G <= steps <= G * (G + 1) // 2
        if margin > 0:
            assert margin >= 1e-3
            assert np.array_equal(mq.numpy()[g[f"{case}:cols:{l}:{b}"]], g[f"{case}:rows:{l}:{b}"]), "the unique optimum"


def test_host_solver_on_random_problems():
    scipy_opt = pytest.importorskip("scipy.optimize")
    rng = np.random.default_rng(5)
    for i in range(200):
        G, Q = int(rng.integers(0, 40)), int(rng.integers(1, 40))
        kind = i % 4
        if kind == 0:
            c = rng.normal(size=(G, Q))
        elif kind == 1:
            c = rng.integers(0, 4, size=(G, Q)).astype(np.float64)                  # many ties
        elif kind == 2:
            c = np.where(rng.random((G, Q)) < 0.15, rng.choice([-100.0, 100.0], size=(G, Q)), rng.normal(size=(G, Q)))
        else:
            c = np.repeat(rng.normal(size=(1, Q)), G, axis=0)                       # duplicate rows
        c = torch.from_numpy(c.astype(np.float32))
        mq, mg, u, v, _ = lsap_host(cost_gq=c) if i % 2 else lsap_host(cost_qg=c.t().contiguous())
        r, cc = scipy_opt.linear_sum_assignment(c.double().numpy())
        want = float(c.double().numpy()[r, cc].sum())
        pairs = [(gi, int(q)) for gi, q in enumerate(mq) if q >= 0]
        assert len(pairs) == min(G, Q) == len({q for _, q in pairs}) and all(int(mg[q]) == gi for gi, q in pairs)
        total = float(sum(c.double()[gi, q] for gi, q in pairs))
        assert abs(total - want) <= 1e-9 * max(1.0, abs(want)), (i, G, Q)
        if G <= Q and G > 0:
            LR.check_certificate(c, mq, u, v)
        elif G > Q:                                                                 # the roles swap: boxes are the spare side
            slack = c.double() - u[:, None] - v[None, :]
            assert float(slack.min()) >= -1e-9 and all(abs(float(slack[gi, q])) <= 1e-9 for gi, q in pairs)
            assert float(u.max()) <= 1e-9 and bool((u[mq < 0] == 0).all())


@pytest.mark.parametrize("case", LR.CASES)
def test_assign_returns_the_references_conventions(g, case):
    a = losses.build_assigner(LR.ASSIGNER)
    cw = torch.tensor(LR.CODE_WEIGHTS)
    Q = int(g[f"{case}:Q"])
    for l, b, margin in LR.problems(g, case):
        if margin == 0:
            continue
        box, cls, gt, lab = assigner_inputs(g, case, l, b)
        inds, labels = a.assign(box, cls, gt, lab, None, cw, True)
        want_inds, want_labels = np.zeros(Q, np.int64), np.full(Q, -1, np.int64)
        rows, cols = g[f"{case}:rows:{l}:{b}"], g[f"{case}:cols:{l}:{b}"]
        want_inds[rows], want_labels[rows] = cols + 1, lab.numpy()[cols]
        assert inds.dtype == labels.dtype == torch.long
        assert np.array_equal(inds.numpy(), want_inds) and np.array_equal(labels.numpy(), want_labels)
    if case == "a":                                                                 # no box: all background, labels -1
        box, cls, gt, lab = assigner_inputs(g, "a", 0, 1)
        inds, labels = a.assign(box, cls, gt, lab, None, cw, True)
        assert bool((inds == 0).all()) and bool((labels == -1).all()) and inds.shape == (Q,)


def test_non_polar_assigner_is_the_same_without_theta(g):
    cfg = {k: v for k, v in LR.ASSIGNER.items() if k != "theta_cost"}
    a, p = losses.build_assigner(dict(cfg, type="HungarianAssigner3D")), losses.build_assigner(LR.ASSIGNER)
    box, cls, gt, lab = assigner_inputs(g, "a", 0, 0)
    cw = torch.tensor(LR.CODE_WEIGHTS)
    theta = p.theta_cost(box * cw, losses.normalize_bbox(gt) * cw)
    assert torch.allclose(a.cost(box, cls, gt, lab, cw, True) + theta, p.cost(box, cls, gt, lab, cw, True), atol=1e-5)
    assert a.fusable() and p.fusable()


@pytest.mark.parametrize("case", LR.CASES)
def test_head_loss_reproduces_the_reference(g, case):
    head = LR.loss_head(int(g[f"{case}:Q"]))
    gts, labels, preds, leaves = LR.case_inputs(g, case)
    boxes_as_objects = [type("Boxes", (), {"gravity_center": t[:, :3], "tensor": t})() for t in gts]
    out = head.loss(boxes_as_objects if case == "a" else gts, labels, preds)
    want = sorted(k.split(":", 2)[2] for k in g if k.startswith(f"{case}:loss64:"))
    assert sorted(out) == want and len(want) == 4 * LR.L
    for k in want:
        LR.assert_close(f"{case} {k}", out[k].detach().numpy(), g[f"{case}:loss32:{k}"], g[f"{case}:loss64:{k}"])
    sum(out.values()).backward()
    for k, leaf in leaves.items():
        LR.assert_close(f"{case} grad {k}", leaf.grad.numpy(), g[f"{case}:grad32:{k}"], g[f"{case}:grad64:{k}"])
    unfused = head.loss_unfused(gts, labels, preds)
    assert all(torch.equal(unfused[k], out[k]) for k in want), "CPU tensors take loss_unfused"


def test_pieces_of_the_reference_interface(g):
    head = LR.loss_head(70)
    gts, labels, preds, _ = LR.case_inputs(g, "a")
    cls, box = preds["all_cls_scores"][1].detach(), preds["all_bbox_preds"][1].detach()
    lab, lw, bt, bw, pos, neg = head._get_target_single(cls[0], box[0], labels[0], gts[0])
    rows, cols = g["a:rows:1:0"], g["a:cols:1:0"]
    assert sorted(pos.tolist()) == sorted(rows.tolist()) and pos.numel() + neg.numel() == 70
    assert bool((lab[neg] == LR.NUM_CLASSES).all()) and np.array_equal(lab.numpy()[rows], labels[0].numpy()[cols])
    assert bt.shape == (70, 9) and torch.equal(bt[torch.from_numpy(rows)], gts[0][torch.from_numpy(cols)]) and bool((bw[pos] == 1).all())
    targets = head.get_targets([cls[0], cls[1]], [box[0], box[1]], gts, labels)
    assert targets[4] == 5 and targets[5] == 2 * 70 - 5
    lc, lb = head.loss_single(cls, box, gts, labels)
    assert lc.numel() == 1 and lb.numel() == 1
    with pytest.raises(NotImplementedError):
        LR.RaCFormer_head(num_classes=10, in_channels=32, num_query=70, bbox_coder=dict(type="NMSFreeCoder", pc_range=LR.PC_RANGE),
                          loss_iou=dict(type="GIoULoss", loss_weight=2.0))


def test_losses_match_their_formulas():
    gen = torch.Generator().manual_seed(2)
    x, t = torch.randn(6, 4, generator=gen), torch.tensor([0, 4, 2, 4, 4, 1])
    onehot = torch.nn.functional.one_hot(t, 5)[:, :4].float()
    p = x.sigmoid()
    pt = (1 - p) * onehot + p * (1 - onehot)
    want = (torch.nn.functional.binary_cross_entropy_with_logits(x, onehot, reduction="none")
            * (0.25 * onehot + 0.75 * (1 - onehot)) * pt ** 2).sum() / (3 + torch.finfo(torch.float32).eps) * 2.0
    assert torch.allclose(losses.FocalLoss(loss_weight=2.0)(x, t, torch.ones(6), avg_factor=3), want)
    a, b, w = torch.randn(5, 10, generator=gen), torch.randn(5, 10, generator=gen), torch.rand(5, 10, generator=gen)
    assert torch.allclose(losses.L1Loss(loss_weight=0.25)(a, b, w, avg_factor=2.0), ((a - b).abs() * w).sum() / (2.0 + torch.finfo(torch.float32).eps) * 0.25)
    empty = losses.L1Loss()(a[:0].requires_grad_(), b[:0], w[:0], avg_factor=1.0)
    assert float(empty) == 0.0 and empty.requires_grad
