"""RaCFormer's training branch of ``extract_feat`` on the CPU (synthetic.SMALL, every part on its torch route): the opt-in switch, what
it refuses, and the branch against the submodules composed by hand (tests/detector_train_ref.py) under the same numpy and torch seeds
-- the per-frame modes, the statistics updated once, which frames carry gradient to which parameters.  (The loss half needs the
decoder, which has no CPU route: tests/test_detector_train_gpu.py.)"""
import copy

import numpy as np
import pytest
import torch

import detector_ref as DR
import detector_train_ref as TR
from racformer_amd import synthetic as syn
from racformer_amd.detector import TRAINING_MESSAGE

CFG = syn.SMALL
SEED = 5


@pytest.fixture(scope="module")
def det():
    return DR.build(CFG)


@pytest.fixture(scope="module")
def step(det):
    """One training-mode ``extract_feat`` and, from the same weights and seeds, the hand composition: computed once, shared."""
    state = copy.deepcopy(det.state_dict())
    det.fused_grad = True
    det.train()
    # the hand composition first: loading a state dict afterwards bumps the parameters' versions, which would break the graph of
    # whatever was computed before it -- and the graph of the call under test is what the gradient tests walk
    b = TR.train_args(CFG)
    TR.seed_all(SEED)
    want = TR.hand_extract_feat_train(det, **TR.feat_args(b))
    hand_next_rand = np.random.rand()
    hand_after = copy.deepcopy(det.state_dict())
    det.load_state_dict(state)
    a = TR.train_args(CFG)
    seen = []
    hook = det.img_lss_view_transformer.register_forward_pre_hook(lambda mod, args: seen.append((args, mod.training, torch.is_grad_enabled())))
    TR.seed_all(SEED)
    try:
        got = det.extract_feat(**TR.feat_args(a))
    finally:
        hook.remove()
    next_rand = np.random.rand()
    modes_after = {n: m.training for n, m in det.named_modules()}
    after = copy.deepcopy(det.state_dict())
    yield dict(got=got, want=want, args=a, seen=seen, before=state, after=after, hand_after=hand_after, modes_after=modes_after,
               rands=(next_rand, hand_next_rand))
    det.fused_grad = False
    det.eval()
    det.load_state_dict(state)


def test_switch_off_refuses_as_before():
    det = DR.build(CFG)
    assert det.fused_grad is False and "training-mode BatchNorm" in TRAINING_MESSAGE and "fused_grad" in TRAINING_MESSAGE
    a = TR.train_args(CFG)
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
        det.forward_train(**a)
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
        det(return_loss=True, **a)
    det.train()
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
        det.extract_feat(**TR.feat_args(a))


def test_switch_reaches_the_parts_and_nothing_else():
    det = DR.build(CFG)
    parts = (det.img_backbone, det.img_neck, det.img_lss_neck, det.radar_encoder)
    assert not any(p.fused_grad for p in parts)
    mix = [m for m in det.modules() if hasattr(m, "fused_linear_grad")]
    before = [m.fused_linear_grad for m in mix]
    det.fused_grad = True
    assert det.fused_grad is True and all(p.fused_grad for p in parts) and [m.fused_linear_grad for m in mix] == before
    det.fused_grad = False
    assert not any(p.fused_grad for p in parts)
    # the reference's attributes; the grid mask adds no state-dict key
    assert det.use_grid_mask is True and type(det.color_aug).__name__ == "GpuPhotoMetricDistortion" and (det.grid_mask.ratio, det.grid_mask.prob) == (0.5, 0.7)
    assert not any(k.startswith("grid_mask") or k.startswith("color_aug") for k in det.state_dict())


def test_stop_prev_grad_is_refused_by_name():
    det = DR.build(CFG, model=dict(DR.small_model(CFG), stop_prev_grad=1))
    det.fused_grad = True
    det.train()
    with pytest.raises(NotImplementedError, match="stop_prev_grad"):
        det.extract_feat(**TR.feat_args(TR.train_args(CFG)))
    det.eval()
    det.extract_feat(**TR.feat_args(TR.train_args(CFG)))     # (outside training the switch changes nothing)


def test_forward_train_needs_training_mode():
    det = DR.build(CFG)
    det.fused_grad = True
    with pytest.raises(RuntimeError, match="train\\(\\)"):
        det.forward_train(**TR.train_args(CFG))


def test_extract_feat_is_the_hand_composition(step):
    T, N = CFG.num_frames, CFG.num_cams
    feats, bev, radar, depth = step["got"]
    assert [tuple(f.shape) for f in feats] == [(1, T * N, 256, h, w) for h, w in CFG.fpn_hw]
    assert tuple(bev.shape) == (1, T, 256, 16, 16) and tuple(radar.shape) == (1, T, 256, 16, 16) and tuple(depth.shape) == (N, DR.D_SMALL, 4, 11)
    want = step["want"]
    for g, w in zip(list(feats) + [bev, radar, depth], list(want[0]) + list(want[1:])):
        assert g.shape == w.shape and torch.equal(g, w)
    assert step["rands"][0] == step["rands"][1], "another number of numpy draws than the hand composition's"
    for k, v in step["after"].items():
        assert torch.equal(v, step["hand_after"][k]), k
    m = step["args"]["img_metas"][0]
    assert m["input_shape"] == (64, 176) and m["pad_shape"][0] == (64, 176, 3) and m["ori_shape"][0] == (64, 176, 3)
    assert all(t.requires_grad for t in list(feats) + [bev, radar, depth])


def test_augmentation_is_live(det, step):
    """The pyramid differs from the eval branch's on the same images: colour distortion and grid mask were applied."""
    det.eval()
    try:
        plain = det.extract_feat(**TR.feat_args(TR.train_args(CFG)))[0]
    finally:
        det.train()
    assert not torch.allclose(plain[0], step["got"][0][0], atol=1e-3)


def test_statistics_move_exactly_once(step):
    before, after = step["before"], step["after"]
    tracked = [k for k in before if k.endswith("num_batches_tracked")]
    branch = [k for k in tracked if k.startswith(("img_lss_view_transformer.", "radar_voxel_encoder.", "radar_bev_conv."))]
    assert len(branch) >= 5 and any(k.startswith("img_lss_view_transformer.depth_net") for k in branch)
    for k in tracked:
        assert int(after[k]) - int(before[k]) == (1 if k in branch else 0), k
    moved = [k for k in before if k.endswith("running_mean") and not torch.equal(before[k], after[k])]
    assert moved and all(k.startswith(("img_lss_view_transformer.", "radar_voxel_encoder.", "radar_bev_conv.")) for k in moved)


def test_frame_modes(step):
    seen = step["seen"]
    assert [(training, grad) for _, training, grad in seen] == [(True, True)] + [(False, False)] * (CFG.num_frames - 1)


def test_later_frames_are_eval_on_the_updated_statistics(det, step):
    _, bev, radar, _ = step["got"]
    a = step["args"]
    det.eval()
    try:
        with torch.no_grad():
            for i in range(1, CFG.num_frames):
                args = step["seen"][i][0]
                again, _ = det.img_lss_view_transformer(*args)
                assert torch.equal(again, bev[:, i])
                assert torch.equal(det.extract_pts_feat(a["radar_points"][i]), radar[:, i])
            first, _ = det.img_lss_view_transformer(*step["seen"][0][0])
            assert not torch.equal(first, bev[:, 0])          # frame 0 ran on batch statistics
    finally:
        det.train()


def branch_params(det):
    return {n: p for n, p in det.named_parameters()
            if n.startswith(("img_lss_view_transformer.", "radar_voxel_encoder.", "radar_bev_conv.")) and p.requires_grad}


def test_which_frames_reach_which_parameters(det, step):
    feats, bev, radar, depth = step["got"]
    params = branch_params(det)
    names, plist = list(params), list(params.values())
    assert len(names) > 20
    # frames >= 1 were computed under no_grad: nothing of them reaches the two branches
    for stack in (bev, radar):
        grads = torch.autograd.grad(stack[:, 1].sum(), plist, retain_graph=True, allow_unused=True)
        assert all(g is None or not bool(g.any()) for g in grads)
    # frame 0 gives every parameter of its branch a gradient
    gb = torch.autograd.grad(bev[:, 0].sum() + depth.sum(), plist, retain_graph=True, allow_unused=True)
    gr = torch.autograd.grad(radar[:, 0].sum(), plist, retain_graph=True, allow_unused=True)
    for n, a, b in zip(names, gb, gr):
        g = a if n.startswith("img_lss_view_transformer.") else b
        assert g is not None and bool(torch.isfinite(g).all()), n
    assert sum(bool(g.any()) for g in gb if g is not None) > 10 and sum(bool(g.any()) for g in gr if g is not None) >= 6
    # the pyramid carries gradient to the backbone for every frame
    N = CFG.num_cams
    w = det.img_backbone.layer4[2].conv3.weight
    for t in range(CFG.num_frames):
        w.grad = None           # (.backward(), not autograd.grad: the backbone's with_cp checkpoints do not support the latter)
        feats[3][:, t * N:(t + 1) * N].sum().backward(retain_graph=True)
        assert w.grad is not None and bool(torch.isfinite(w.grad).all()) and bool(w.grad.any()), t
    det.zero_grad(set_to_none=True)


def test_modes_afterwards(det, step):
    modes = step["modes_after"]
    assert modes[""] is True
    bns = [n for n, m in det.img_backbone.named_modules() if isinstance(m, torch.nn.BatchNorm2d)]
    assert bns
    for n, training in modes.items():
        if n.startswith("img_backbone.") and n[len("img_backbone."):] in bns:
            assert training is False, n              # norm_eval
        elif not n.startswith("img_backbone."):
            assert training is True, n
    assert det.radar_encoder.training is True
    assert det.img_backbone.input_norm == DR.NORM and det.pregrouped is True


def test_a_frozen_submodule_stays_frozen():
    """The departure from the reference's ``self.eval()`` / ``self.train()``: a part the user put into eval() is in eval() afterwards."""
    det = DR.build(CFG)
    det.fused_grad = True
    det.train()
    det.img_neck.eval()
    det.pts_bbox_head.eval()
    TR.seed_all(SEED)
    with torch.no_grad():
        det.extract_feat(**TR.feat_args(TR.train_args(CFG)))
    assert not det.img_neck.training and not det.pts_bbox_head.training and det.img_lss_view_transformer.training
