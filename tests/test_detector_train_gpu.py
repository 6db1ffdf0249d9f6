"""RaCFormer.forward_train on the MI355X at synthetic.SMALL (T = 3), B = 1 and B = 2 (samples with different box counts, one without
a box): the losses against the device submodules composed by hand (tests/detector_train_ref.py) under the same numpy and torch seeds
-- bitwise, every forward kernel here is reproducible --, the backward of the summed losses per parameter, and inference after the step.

Gradients cannot be bitwise: the feature and value scatters of the two gather backwards use atomics.  Their bound is measured, not
chosen (per batch size; relative L2 per parameter, the largest over the parameters that have a gradient to speak of -- NOISE_ONLY
below lists the others by name, with the reason, and they get a check of their own):
  spread   two runs of the hand composition against each other (floored at one float32 rounding, 2^-24: two runs that happen to
           agree to the bit say nothing about the next pair)
  faults   three wiring faults built into the hand composition on purpose, each against the hand composition: frame 1's branches
           under autograd, frame 0's branches in eval mode, the grid mask dropped
  bound    the geometric mean of the spread and the smallest fault
The detector's gradients lie within the bound of the hand composition's and every fault lies beyond it, which proves the comparison
would catch them.  With RAC_DETECTOR_TRAIN_ERRORS=<file> the figures, the parameter at which each maximum sits and the five largest
entries of every measure are written there (committed copy: profiles/detector_train_small.json).

Measured on an MI355X (B = 1 / B = 2): spread 1.5e-6 / 1.2e-6 and detector 1.6e-6 / 1.2e-6, both in backbone stage 2; faults 20 / 36
(frame 1 under autograd), 397 / 281 (frame 0 in eval mode), 1.8 / 1.3 (no grid mask); bound 1.7e-3 / 1.3e-3; the noise-only bias at
7e-11 / 1.5e-10 of its weight's gradient."""
import copy
import json
import math
import os

import pytest
import torch

import detector_ref as DR
import detector_train_ref as TR
from racformer_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = syn.SMALL
SEED = 7
COUNTS = {1: (3,), 2: (2, 0)}
FAULTS = ("frame1_autograd", "frame0_eval", "no_grid_mask")
FIGURES = {}
_RUNS = {}

# Parameters with requires_grad that the summed losses cannot reach, by name prefix, with the reason.  None at this configuration: the
# depth loss and the BEV map reach all of the view transformer, the radar stack reaches all of the radar branch, the four pyramid
# levels reach backbone stages 2-4 and both necks, every decoder layer is supervised (d0 .. d4 and the last), and the denoising queries
# reach label_enc.  (Measured: 324 of 359 parameters get a gradient; the other 35 are the frozen stem and stage 1, code_weights and the frustum.)
UNREACHED = {
}

# Parameters whose TRUE gradient is zero although the losses reach them: what autograd returns for them is the rounding of a sum that
# cancels, and two runs differ by about its own size, so a relative difference says nothing.  name -> (reason, the weight of the same
# layer).  They are left out of the relative-L2 maximum and checked against the scale of that weight's gradient instead.
# (Found on the CPU route, where the gradient of this bias is 1e-10 of its weight's; every other bias of the two branches is within a
# factor of twenty of its weight's gradient.)
NOISE_ONLY = {
    "img_lss_view_transformer.depth_net.reduce_conv.0.bias":
        ("a convolution bias directly in front of a batch-statistics BatchNorm (frame 0 trains): the normalisation subtracts the "
         "channel mean, so the output does not depend on the bias", "img_lss_view_transformer.depth_net.reduce_conv.0.weight"),
}
# ||grad bias|| <= NOISE_RATIO x ||grad weight||: the bias gradient is the per-channel sum over n = B * N * h * w <= 264 pixels of a
# gradient map whose exact sum is zero; float32 summation leaves at most about n * 2^-24 = 1.6e-5 of the terms' magnitude, and the weight
# gradient -- 9 * 256 products of the same terms with O(1) activations per output channel -- is no smaller than the terms.
NOISE_RATIO = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    path = os.environ.get("RAC_DETECTOR_TRAIN_ERRORS")
    if path and FIGURES:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(FIGURES, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def rig():
    det = DR.build(CFG).to(DEV)
    det.fused_grad = True
    det.train()
    return det, copy.deepcopy(det.state_dict())


def run(rig, B, how, fault=None):
    """One forward + backward of the summed losses from the rig's initial state under the fixed seeds -> (losses, gradients by name);
    computed once per (B, how, fault) except for the repeats ("det2", "hand2"), shared, not modified."""
    key = (B, how, fault)
    if key in _RUNS:
        return _RUNS[key]
    det, state = rig
    det.load_state_dict(state)
    det.zero_grad(set_to_none=True)
    a = TR.train_args(CFG, COUNTS[B], device=DEV)
    TR.seed_all(SEED)
    losses = det(return_loss=True, **a) if how.startswith("det") else TR.hand_forward_train(det, a, fault)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    grads = {n: (p.grad.detach().clone() if p.grad is not None else None) for n, p in det.named_parameters()}
    _RUNS[key] = ({k: v.detach().clone() for k, v in losses.items()}, grads, a)
    det.zero_grad(set_to_none=True)
    return _RUNS[key]


def rel_l2(grads, ref):
    """The largest relative L2 difference over the parameters (NOISE_ONLY left out), its name, and the five largest entries."""
    worst, where, every = 0.0, None, []
    for n, g in ref.items():
        if n in NOISE_ONLY:
            continue
        o = grads[n]
        if g is None and o is None:
            continue
        # (a gradient that is missing on one side counts as zeros: a fault may cut a parameter off)
        g = torch.zeros_like(o) if g is None else g
        o = torch.zeros_like(g) if o is None else o
        den = float(g.double().norm())
        num = float((o.double() - g.double()).norm())
        r = num / den if den > 0 else (0.0 if num == 0 else math.inf)
        every.append((r, n))
        if r > worst:
            worst, where = r, n
    return worst, where, [dict(parameter=n, rel_l2=r) for r, n in sorted(every, reverse=True)[:5]]


@pytest.mark.parametrize("B", [1, 2])
def test_losses(rig, B):
    det = rig[0]
    losses, _, a = run(rig, B, "det")
    L = CFG.num_layers
    want_keys = {"loss_depth", "loss_cls", "loss_bbox"} | {f"d{i}.loss_{k}" for i in range(L - 1) for k in ("cls", "bbox")}
    want_keys |= {k + "_dn" for k in want_keys if k != "loss_depth"}
    assert set(losses) == want_keys
    assert all(v.dim() == 0 and v.is_cuda and bool(torch.isfinite(v)) for v in losses.values())
    assert float(losses["loss_depth"]) > 0 and float(losses["loss_cls"]) > 0 and float(losses["loss_bbox_dn"]) > 0
    assert all("gt_bboxes_3d" in m and m["input_shape"] == (64, 176) for m in a["img_metas"])
    hand, _, _ = run(rig, B, "hand")
    again, _, _ = run(rig, B, "det2")
    for k in losses:
        assert torch.equal(losses[k], hand[k]), f"{k}: {float(losses[k])!r} against the hand composition's {float(hand[k])!r}"
        assert torch.equal(losses[k], again[k]), f"{k}: two seeded runs differ"
    assert det.training and det.pts_bbox_head.transformer.decoder.pregrouped is False


@pytest.mark.parametrize("B", [1, 2])
def test_gradients(rig, B):
    det = rig[0]
    _, grads, _ = run(rig, B, "det")
    frozen = [n for n, p in det.named_parameters() if not p.requires_grad]
    stem = [n for n in frozen if n.startswith("img_backbone.")]
    assert stem and all(n.split(".")[1] in ("conv1", "bn1", "layer1") for n in stem)           # frozen_stages=1
    # (the other two: a constant of the loss and the frustum, a geometry table kept as a parameter)
    assert set(frozen) - set(stem) == {"pts_bbox_head.code_weights", "img_lss_view_transformer.frustum"}
    missing, reached = [], 0
    for n, p in det.named_parameters():
        g = grads[n]
        if not p.requires_grad:
            assert g is None, f"{n}: frozen (frozen_stages=1), yet it has a gradient"
            continue
        if any(n.startswith(pre) for pre in UNREACHED):
            assert g is None or not bool(g.any()), f"{n}: listed as unreachable, yet it has a gradient"
            continue
        if n in NOISE_ONLY:
            assert g is not None and bool(torch.isfinite(g).all()), n
            continue
        if g is None or not bool(torch.isfinite(g).all()) or not bool(g.any()):
            missing.append(n)
        else:
            reached += 1
    print(f"B={B}: {reached} parameters reached; without a finite non-zero gradient: {missing}")
    assert not missing and reached > 100

    _, hand, _ = run(rig, B, "hand")
    _, hand2, _ = run(rig, B, "hand2")
    spread, spread_at, spread_top = rel_l2(hand2, hand)
    effects, effects_at, top = {}, {}, dict(spread=spread_top)
    for fault in FAULTS:
        effects[fault], effects_at[fault], top[fault] = rel_l2(run(rig, B, "hand", fault)[1], hand)
    floor = 2.0 ** -24
    bound = math.sqrt(max(spread, floor) * min(effects.values()))
    err, err_at, top["detector"] = rel_l2(grads, hand)
    noise = {}
    for n, (_, weight) in NOISE_ONLY.items():
        for who, gr in (("detector", grads), ("hand", hand), ("hand2", hand2)):
            noise[f"{n}:{who}"] = float(gr[n].double().norm()) / float(gr[weight].double().norm())
    FIGURES[f"B{B}"] = dict(spread=spread, spread_at=spread_at, faults=effects, faults_at=effects_at, bound=bound, detector=err,
                            detector_at=err_at, five_largest=top, noise_only_over_weight_gradient=noise, noise_ratio_allowed=NOISE_RATIO)
    print(f"B={B}: run-to-run spread {spread:.3g} ({spread_at}), faults {effects} at {effects_at}, bound {bound:.3g}, "
          f"detector {err:.3g} ({err_at}); noise-only parameters over their weight's gradient {noise}")
    assert all(v <= NOISE_RATIO for v in noise.values()), f"a gradient whose true value is zero is not small: {noise}"
    assert err <= bound, f"gradient of {err_at}: relative L2 {err:.3g} against the hand composition's, allowed {bound:.3g}"
    for fault, e in effects.items():
        assert e > bound, f"the comparison would not catch '{fault}': its effect {e:.3g} is within the bound {bound:.3g}"


def test_inference_after_the_step(rig):
    det, state = rig
    run(rig, 1, "det")
    det.load_state_dict(state)
    a = TR.train_args(CFG, COUNTS[1], device=DEV)
    TR.seed_all(SEED)
    sum(det.forward_train(**a).values()).backward()
    opt = torch.optim.SGD([p for p in det.parameters() if p.requires_grad and p.grad is not None], lr=1e-4)
    opt.step()
    det.zero_grad(set_to_none=True)
    det.eval()
    try:
        res = det.simple_test_offline(**DR.offline_args(CFG, [2, 1, 0], device=DEV))
        assert res[0]["pts_bbox"]["boxes_3d"].shape[1] == 9 and res[0]["pts_bbox"]["boxes_3d"].shape[0] > 0
        assert det.pts_bbox_head.transformer.decoder.pregrouped is True
        assert det.memory is None and det._plan is None             # the step emptied the streaming memory
        replayed = []
        for s, fids in enumerate(DR.sequence(2, CFG.num_frames)):
            img, points, depth, rcs, metas = DR.window_inputs(CFG, fids, sample=s, device=DEV)
            got = det.simple_test_online(metas, img, False, points, depth, rcs)
            replayed.append(det._plan is not None)
            assert got[0]["pts_bbox"]["boxes_3d"].shape[0] > 0
        assert replayed == [False, True]
        # the head's weights change: the plan captured on the old ones is dropped and a new one captured
        old = det._plan
        moved = copy.deepcopy(det.state_dict())
        moved["pts_bbox_head.init_query_bbox.weight"] *= 1.0
        det.load_state_dict(moved)                                  # (train() and load_state_dict make the next call look at the weights)
        img, points, depth, rcs, metas = DR.window_inputs(CFG, DR.sequence(3, CFG.num_frames)[2], sample=2, device=DEV)
        det.simple_test_online(metas, img, False, points, depth, rcs)
        assert det._plan is not None and det._plan is not old and old.graph is None
    finally:
        det.reset_memory()
        det.train()
        det.load_state_dict(state)


def test_gt_depth_of_another_size_is_refused(rig):
    det, state = rig
    det.load_state_dict(state)
    a = TR.train_args(CFG, COUNTS[1], device=DEV)
    a["gt_depth"] = a["gt_depth"][..., :160]
    with pytest.raises(ValueError, match="gt_depth"):
        det.forward_train(**a)
    det.load_state_dict(state)
