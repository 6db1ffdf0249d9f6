"""What the head-loss edge tests share (tests/test_head_loss_edges_cpu.py, tests/test_head_loss_edges_gpu.py): float64 torch
restatements of the match cost and of the focal + L1 sums with their gradients, written from the formulas and independent of
match.hip / det_loss.hip (they also run in float32, for the rounding figure of the comparison rule); seeded generators of
assignment problems at the shapes the fixture never reaches; the kernels' [P, Gmax, Qpad] layout; seeded inputs of the match-cost
and detection-loss tests with their planted edges.  The comparison rule is loss_ref.assert_close's: the kernel against float64
within bound(e32), e32 the same restatement in float32 against float64."""
import math
import zlib

import numpy as np
import torch
import torch.nn.functional as F

import loss_ref as LR
from decoder_grad_ref import bound

L = 2
TWO_PI = 2.0 * math.pi
NAN, INF = float("nan"), float("inf")


# ------------------------------------------------------------------------------------------------ the formulas
def normalize_gt(gt):
    """[n,9] x, y, z, w, l, h, yaw, vx, vy -> [n,10] cx, cy, log w, log l, cz, log h, sin, cos, vx, vy"""
    return torch.stack([gt[:, 0], gt[:, 1], gt[:, 3].log(), gt[:, 4].log(), gt[:, 2], gt[:, 5].log(), gt[:, 6].sin(), gt[:, 6].cos(),
                        gt[:, 7], gt[:, 8]], dim=1)


def theta_turns(xy):
    """ThetaL1Cost's polar angle in turns of code-weighted centres [n, >= 2], through its fixed +-51.2 normalisation"""
    nx, ny = (xy[:, 0] + 51.2) / 102.4, (xy[:, 1] + 51.2) / 102.4
    dx, dy = nx * 102.4 - 51.2, ny * 102.4 - 51.2
    return torch.remainder(torch.atan2(dy, dx) + TWO_PI, TWO_PI) / TWO_PI


def cost_ref(cls, box, gt, labels, code_weights, w_cls, w_reg, w_theta, dtype=torch.float64):
    """cls [Q,C] logits, box [Q,10], gt [G,9], labels [G] -> the match cost [G,Q] (the kernels' orientation):
    FocalLossCost (alpha 0.25, gamma 2, eps 1e-12) + L1 of the code-weighted prediction against the code-weighted
    normalize_bbox(gt) (+ ThetaL1Cost, w_theta None: without), nan_to_num(100, 100, -100).  A label outside 0..C-1 has no class
    cost (NaN): its row is 100 throughout."""
    cls, box, gt, cw = (torch.as_tensor(t).detach().cpu().to(dtype) for t in (cls, box, gt, code_weights))
    labels = torch.as_tensor(labels).detach().cpu().long()
    C = cls.shape[1]
    p = cls.sigmoid()
    pos = -(p + 1e-12).log() * 0.25 * (1 - p) ** 2
    neg = -(1 - p + 1e-12).log() * 0.75 * p ** 2
    cost = ((pos - neg) * w_cls)[:, labels.clamp(0, C - 1)].t().clone()
    cost[(labels < 0) | (labels >= C)] = NAN
    pb, tb = box * cw, normalize_gt(gt) * cw
    cost = cost + (tb[:, None, :] - pb[None, :, :]).abs().sum(-1) * w_reg
    if w_theta is not None:
        d = (theta_turns(tb)[:, None] - theta_turns(pb)[None, :]).abs()
        cost = cost + (torch.remainder(d + 0.5, 1.0) - 0.5).abs() * w_theta
    return torch.nan_to_num(cost, nan=100.0, posinf=100.0, neginf=-100.0)


def det_loss_ref(logits, boxes, target, gt, labels, code_weights, alpha, gamma, dtype=torch.float64):
    """logits [L,R,C], boxes [L,R,10], target [L,R] (index into gt, -1 background) or None (row r takes r mod len(gt)), gt [n,9],
    labels [n] -> (sums [L,2], d sums / d logits, d sums / d boxes) by autograd on the textbook formulas: BCE-with-logits x
    (alpha t + (1 - alpha)(1 - t)) x pt^gamma with pt = 1 - p on the label and p elsewhere (written sigmoid(-x) and sigmoid(x));
    |box - normalize_bbox(gt)| x code weight.  Background rows: all-zero one-hot, no box term; a positive row whose normalised
    target has a non-finite entry: no box term."""
    x = torch.as_tensor(logits).detach().cpu().to(dtype).requires_grad_()
    bx = torch.as_tensor(boxes).detach().cpu().to(dtype).requires_grad_()
    gt, cw = (torch.as_tensor(t).detach().cpu().to(dtype) for t in (gt, code_weights))
    labels = torch.as_tensor(labels).detach().cpu().long()
    nl, R, C = x.shape
    n = gt.shape[0]
    if target is None:
        tgt = (torch.arange(R) % n).expand(nl, R) if n > 0 else torch.full((nl, R), -1, dtype=torch.long)
    else:
        tgt = torch.as_tensor(target).detach().cpu().long()
    positive = (tgt >= 0) & (tgt < n)
    idx = torch.where(positive, tgt, torch.zeros_like(tgt))
    if n > 0:
        label = torch.where(positive, labels[idx], torch.full_like(tgt, C))
        tb = normalize_gt(gt)[idx]                                              # [L,R,10]
    else:
        label, tb = torch.full_like(tgt, C), torch.zeros(nl, R, 10, dtype=dtype)
    t = F.one_hot(label.clamp(0, C), C + 1)[..., :C].to(dtype)
    pt = torch.sigmoid((1 - 2 * t) * x)
    focal = F.binary_cross_entropy_with_logits(x, t, reduction="none") * (alpha * t + (1 - alpha) * (1 - t)) * pt.pow(gamma)
    use = (positive & torch.isfinite(tb).all(-1))[..., None]
    l1 = (bx - torch.where(use, tb, torch.zeros_like(tb))).abs() * cw * use.to(dtype)
    sums = torch.stack([focal.sum((1, 2)), l1.sum((1, 2))], dim=1)
    g_logits, g_boxes = torch.autograd.grad(sums.sum(), (x, bx))
    return sums.detach(), g_logits, g_boxes


def figures(what, got, ref32, ref64, mask=None):
    """the comparison rule: prints (kernel figure, float32 reference figure, bound) and asserts the first within the last;
    every entry takes part unless ``mask`` leaves it out"""
    got, ref32, ref64 = (np.asarray(torch.as_tensor(a).detach().cpu().numpy(), dtype=np.float64) for a in (got, ref32, ref64))
    kept = np.ones(ref64.shape, dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
    assert np.isfinite(ref64[kept]).all() and np.isfinite(ref32[kept]).all(), f"{what}: the reference is not finite on a compared entry"
    assert np.isfinite(got[kept]).all(), f"{what}: non-finite where the reference is finite"
    fig, e32 = LR.rel_err(got, ref64, kept), LR.rel_err(ref32, ref64, kept)
    print(f"  {what}: rel err {fig:.3e}, reference float32 {e32:.3e}, bound {bound(e32):.3e}")
    assert fig <= bound(e32), f"{what}: {fig:.3e} > {bound(e32):.3e}"
    return fig, e32


# ------------------------------------------------------------------------------------------------ assignment problems
KINDS = ("normal", "ties", "pinned", "duplicate", "dominant")
# (boxes per sample, Q): Q < 64, Q = 64 and 65, square problems, the workload's Q = 900 (15 queries a lane), the solver's limit
# Q = 2048 (32 a lane), its full LDS carve (G = Q = 2048: the one-step kind only), up to four samples of different sizes a launch
ASSIGN_SHAPES = [((1, 0, 64, 33), 64), ((65, 2), 65), ((5,), 5), ((1,), 1), ((192,), 192), ((120, 300, 17), 900), ((64,), 2048)]
ASSIGN_CASES = [(counts, Q, kind) for counts, Q in ASSIGN_SHAPES for kind in KINDS] + [((2048,), 2048, "dominant")]
_CACHE = {}


def problem(kind, G, Q, rng):
    """-> (cost [G,Q] float32, the planted matching [G] or None)"""
    pi = None
    if kind == "normal":
        c = rng.normal(size=(G, Q))
    elif kind == "ties":
        c = rng.integers(0, 4, size=(G, Q)).astype(np.float64)
    elif kind == "pinned":
        c = np.where(rng.random((G, Q)) < 0.15, rng.choice([-100.0, 100.0], size=(G, Q)), rng.normal(size=(G, Q)))
    elif kind == "duplicate":
        c = np.repeat(rng.normal(size=(1, Q)), G, axis=0)
    elif kind == "dominant":
        # c[g, pi(g)] = -10 + U(0, 0.1), elsewhere U(0, 1), pi an injection: every row's minimum is its own free query, so every
        # augmentation ends in its first step and the duals of the queries stay 0
        pi = rng.permutation(Q)[:G]
        c = rng.random((G, Q), dtype=np.float32)
        c[np.arange(G), pi] = -10.0 + 0.1 * rng.random(G, dtype=np.float32)
    else:
        raise ValueError(kind)
    return torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)), pi


def launch_problems(kind, counts, Q):
    """{(layer, sample): (cost [G,Q] float32, planted matching or None)} of one launch, another matrix per layer; drawn once"""
    key = ("problems", kind, tuple(counts), Q)
    if key not in _CACHE:
        rng = np.random.default_rng(zlib.crc32(f"{kind}:{tuple(counts)}:{Q}".encode()))
        _CACHE[key] = {(l, b): problem(kind, G, Q, rng) for l in range(L) for b, G in enumerate(counts)}
    return _CACHE[key]


def host_solutions(kind, counts, Q):
    """{(layer, sample): lsap_host's (matched_query, matched_gt, u, v, steps)} on the float32 matrices; solved once"""
    from racformer_amd.fused import lsap_host
    key = ("host", kind, tuple(counts), Q)
    if key not in _CACHE:
        _CACHE[key] = {k: lsap_host(cost_gq=c) for k, (c, _) in launch_problems(kind, counts, Q).items() if c.shape[0] > 0}
    return _CACHE[key]


def total_of(cost_gq, matched_query):
    c = torch.as_tensor(cost_gq).double()
    G = c.shape[0]
    return float(c[torch.arange(G), torch.as_tensor(matched_query)[:G].long()].sum())


def lay_out(mats, counts, Q, fill, num_layers=L):
    """{(l, b): [G_b, Q]} -> [num_layers * B, Gmax, Qpad] float32 (Qpad: Q rounded up to 64), everything else ``fill``"""
    B = len(counts)
    out = torch.full((num_layers * B, max(counts), (Q + 63) // 64 * 64), fill, dtype=torch.float32)
    for (l, b), m in mats.items():
        m = m[0] if isinstance(m, tuple) else m
        assert tuple(m.shape) == (counts[b], Q)
        out[l * B + b, :counts[b], :Q] = m
    return out


# ------------------------------------------------------------------------------------------------ match-cost inputs
MC_B, MC_Q, MC_COUNTS = 4, 300, (300, 7, 0, 257)
MC_W0_BOX = (0, 100)          # (sample, box): w = 0, the row is +inf -> 100
MC_BAD_LABEL = (1, 3)         # (sample, box): label = C
MC_NAN_LOGIT = (0, 0, 5)      # (layer, sample, query): NaN in the class of box 258 of that sample (second staging trip)
MC_INF_LOGIT = (1, 3, 299)    # (layer, sample, query): +inf in the class of box 256 of that sample (the 1-box tail)
MC_WRAP = ((0, 0, 17), (1, 3, 270))   # (layer, sample, query): the centre sits a hair below the +x axis


def gt_table(rng, n, C):
    box = np.zeros((n, 9), np.float32)
    quad = np.array([[1, 1], [-1, 1], [-1, -1], [1, -1]], np.float32)[np.arange(n) % 4]
    box[:, 0:2] = rng.uniform(3.0, 48.0, (n, 2)) * quad
    box[:, 2] = rng.uniform(-2.0, 1.0, n)
    box[:, 3:6] = rng.uniform(0.5, 5.0, (n, 3))
    box[:, 6] = rng.uniform(-np.pi, np.pi, n)
    box[:, 7:9] = rng.uniform(-3.0, 3.0, (n, 2))
    return box, rng.integers(0, C, n).astype(np.int32)


def pred_boxes(rng, shape):
    box = np.zeros(shape + (10,), np.float32)
    box[..., 0:2] = rng.uniform(-50.0, 50.0, shape + (2,))
    box[..., 2:4] = rng.uniform(-0.7, 1.7, shape + (2,))
    box[..., 4] = rng.uniform(-2.0, 1.0, shape)
    box[..., 5] = rng.uniform(-0.7, 1.7, shape)
    ang = rng.uniform(-np.pi, np.pi, shape)
    box[..., 6], box[..., 7] = np.sin(ang), np.cos(ang)
    box[..., 8:10] = rng.uniform(-3.0, 3.0, shape + (2,))
    return box


def match_cost_inputs(C):
    """-> dict(cls [L,B,Q,C], box [L,B,Q,10], gt [sum G,9], labels [sum G] int32, off) with the four edges planted"""
    key = ("mc", C)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(900 + C)
    off = np.concatenate([[0], np.cumsum(MC_COUNTS)])
    gt, labels = gt_table(rng, int(off[-1]), C)
    cls = rng.normal(-2.0, 1.5, (L, MC_B, MC_Q, C)).astype(np.float32)
    box = pred_boxes(rng, (L, MC_B, MC_Q))
    gt[off[MC_W0_BOX[0]] + MC_W0_BOX[1], 3] = 0.0
    labels[off[MC_BAD_LABEL[0]] + MC_BAD_LABEL[1]] = C
    l, b, q = MC_NAN_LOGIT
    cls[l, b, q, labels[off[b] + 258]] = np.nan
    l, b, q = MC_INF_LOGIT
    cls[l, b, q, labels[off[b] + 256]] = np.inf
    for l, b, q in MC_WRAP:
        # code weight 2: the weighted centre is (50, -4e-6); one ulp of 51.2 is 3.8e-6, so float32 sees the angle as -7.6e-8
        # or as 0 and either way returns theta = 0 after adding 2 pi, while float64 returns 1 - 1.2e-8
        box[l, b, q, 0], box[l, b, q, 1] = 25.0, -2e-6
    d = dict(cls=torch.from_numpy(cls), box=torch.from_numpy(box), gt=torch.from_numpy(gt), labels=torch.from_numpy(labels),
             off=[int(o) for o in off])
    _CACHE[key] = d
    return d


def match_cost_refs(C, polar):
    """{(l, b): (cost32, cost64) [G,Q]} for the samples with boxes, LR.ASSIGNER's weights; computed once"""
    key = ("mcref", C, polar)
    if key not in _CACHE:
        d, a, out = match_cost_inputs(C), LR.ASSIGNER, {}
        w = (a["cls_cost"]["weight"], a["reg_cost"]["weight"], a["theta_cost"]["weight"] if polar else None)
        for l in range(L):
            for b, G in enumerate(MC_COUNTS):
                if G:
                    args = (d["cls"][l, b], d["box"][l, b], d["gt"][d["off"][b]:d["off"][b + 1]], d["labels"][d["off"][b]:d["off"][b + 1]],
                            LR.CODE_WEIGHTS) + w
                    out[(l, b)] = (cost_ref(*args, dtype=torch.float32), cost_ref(*args, dtype=torch.float64))
        _CACHE[key] = out
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ detection-loss inputs
DL_SHAPES = [(1100, 10), (1100, 1), (1024, 10), (1, 10)]       # (R, C): two ragged trips of the 1024-thread row loop; one full; one row
DL_TARGETS = ("explicit", "modulo", "empty_explicit", "empty_modulo")
DL_FOCAL = [(0.25, 2.0), (0.4, 1.5)]
DL_PLANTED = (30.0, -30.0, 88.0, -88.0, 104.0, -104.0)
DL_H0_BOX = 5                 # gt index with h = 0: its normalised target has -inf
DL_PASS_THROUGH = [0, 1, 4, 8, 9]      # x, y, z, vx, vy are copied by normalize_bbox


def det_loss_inputs(R, C, mode):
    """-> dict(logits [L,R,C], boxes [L,R,10], target [L,R] int32 or None, gt [n,9], labels [n] int32, exact_rows [(l, r)],
    h0_rows [(l, r)], planted: how many of the extreme logits found a label / a non-label position)"""
    key = ("dl", R, C, mode)
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(zlib.crc32(f"dl:{R}:{C}:{mode}".encode()))
    n = {"explicit": 23, "modulo": 7}.get(mode, 0)
    gt, labels = gt_table(rng, n, C)
    if n:
        gt[DL_H0_BOX, 5] = 0.0
    if mode == "explicit":
        tgt = np.where(rng.random((L, R)) < 0.1, rng.integers(0, n, (L, R)), -1)
        tgt[0, 0] = 3
        if R > 1:
            tgt[:, 1] = DL_H0_BOX
            tgt[1, R - 1] = 11                                                    # the last row of the ragged second trip
    elif mode == "modulo":
        tgt = np.broadcast_to(np.arange(R) % n, (L, R)).copy()
    else:
        tgt = np.full((L, R), -1)
    gt_t = torch.from_numpy(gt)
    nb = normalize_gt(gt_t).numpy() if n else np.zeros((0, 10), np.float32)
    boxes = pred_boxes(rng, (L, R))
    exact_rows, h0_rows = [], []
    for l in range(L):
        rows = np.nonzero(tgt[l] >= 0)[0]
        for r in rows:
            if tgt[l, r] == DL_H0_BOX:
                h0_rows.append((l, int(r)))
                continue
            sign = np.where(rng.random(10) < 0.5, -1.0, 1.0)
            boxes[l, r] = nb[tgt[l, r]] + (sign * rng.uniform(0.05, 2.0, 10)).astype(np.float32)      # away from the kink of |d|
        for r in [r for r in rows if tgt[l, r] != DL_H0_BOX][-3:]:             # (the last positives: the second trip where R > 1024)
            boxes[l, r, DL_PASS_THROUGH] = nb[tgt[l, r], DL_PASS_THROUGH]
            exact_rows.append((l, int(r)))
    logits = (3.0 * rng.standard_normal((L, R, C))).astype(np.float32)
    lab = np.where(tgt >= 0, labels[np.maximum(tgt, 0)] if n else C, C)                                # [L,R]
    onehot = lab[..., None] == np.arange(C)
    planted = []
    for where in (onehot, ~onehot):
        flat = np.flatnonzero(where)
        pick = flat[np.linspace(0, len(flat) - 1, num=min(len(flat), len(DL_PLANTED))).astype(int)] if len(flat) else flat
        pick = np.unique(pick)
        logits.reshape(-1)[pick] = np.array(DL_PLANTED, np.float32)[:len(pick)]
        planted.append(len(pick))
    d = dict(logits=torch.from_numpy(logits), boxes=torch.from_numpy(boxes),
             target=torch.from_numpy(tgt.astype(np.int32)) if mode in ("explicit", "empty_explicit") else None,
             gt=gt_t, labels=torch.from_numpy(labels), exact_rows=exact_rows, h0_rows=h0_rows, planted=tuple(planted))
    _CACHE[key] = d
    return d


def det_loss_refs(R, C, mode, alpha, gamma):
    """-> ((sums, g_logits, g_boxes) in float32, the same in float64); computed once"""
    key = ("dlref", R, C, mode, alpha, gamma)
    if key not in _CACHE:
        d = det_loss_inputs(R, C, mode)
        args = (d["logits"], d["boxes"], d["target"], d["gt"], d["labels"], LR.CODE_WEIGHTS, alpha, gamma)
        _CACHE[key] = (det_loss_ref(*args, dtype=torch.float32), det_loss_ref(*args, dtype=torch.float64))
    return _CACHE[key]
