"""The radar pillar branch's training switch without a GPU: the torch route under autograd against the float64 restatement
(tests/radar_pillars_grad_ref.py), the switch's off state, and the argument checks of the new entry points."""
import ctypes

import pytest
import torch

import radar_pillars_grad_ref as G
import radar_pillars_ref as R
from racformer_amd import _lib
from racformer_amd import synthetic as syn
from test_radar_pillars_ref import encoder


def clouds_b2():
    return syn.make_radar_points(2, [300, 120], seed=9, grid=16, edge_fraction=0.2)


def test_7_torch_route_in_training_mode_matches_float64():
    """fused_grad on, CPU tensors: outputs, gradients and buffers of one step, the route's own decisions (taken from its modules'
    outputs by hooks) imposed on the restatement"""
    sd, clouds = R.make_state_dict(71), clouds_b2()
    enc = encoder(R.SMALL, sd).train()
    enc.fused_grad = True
    seen = {}
    layer = enc.radar_voxel_encoder.pfn_layers[0]
    hooks = [layer.norm.register_forward_hook(lambda m, i, o: seen.__setitem__("pre", o.detach().transpose(1, 2)))]
    for i, m in enumerate(enc.radar_bev_conv):
        hooks.append(m.register_forward_hook(lambda m, a, o, i=i: seen.__setitem__(i, o.detach() > 0)))
    out = enc.extract_pts_feat(clouds)
    for h in hooks:
        h.remove()
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(72))
    out.backward(gout)
    v, c, n = R.voxelize_batch(clouds, zero_z=True, **R.SMALL)
    slots = G.first_max_slots(torch.relu(seen["pre"]), n)
    P = v.shape[1]
    win = seen["pre"].gather(1, torch.where(slots < 0, n.long().view(-1, 1).expand(-1, 64).clamp(max=P - 1), slots).unsqueeze(1)).squeeze(1)
    dec = dict(slots=slots, pos=win > 0, masks=[seen[i] for i in range(3)])
    w64 = G.grads_and_buffers(sd, R.SMALL, torch.float64, v, c, n, 2, gout, dec)
    w32 = G.grads_and_buffers(sd, R.SMALL, torch.float32, v, c, n, 2, gout, dec)
    assert out.shape == (2, 256, 16, 16) and out.requires_grad
    G.hold("torch route output", out, w64[0], w32[0])
    named, state = dict(enc.named_parameters()), enc.state_dict()
    for k in G.PARAMS:
        G.hold(f"torch route grad {k}", named[k].grad, w64[1][k], w32[1][k])
    for k in G.BUFFERS:
        if k.endswith("num_batches_tracked"):
            assert int(state[k]) == int(w64[2][k]) == 8
        else:
            G.hold(f"torch route {k}", state[k], w64[2][k], w32[2][k])


def test_7_forward_over_frames_on_the_torch_route():
    """frame 0 trains, frame 1 runs in eval mode on the statistics frame 0 has just updated; the module stays in training mode"""
    sd = R.make_state_dict(71)
    clouds = syn.make_radar_points(4, [300, 120, 0, 200], seed=10, grid=16, edge_fraction=0.2)
    frames = [[clouds[0], clouds[1]], [clouds[2], clouds[3]]]
    enc = encoder(R.SMALL, sd, fused=False).train()
    enc.fused_grad = True
    out = enc(frames)
    assert out.shape == (2, 2, 256, 16, 16) and out.requires_grad and all(m.training for m in enc.modules())
    after = {k: v.clone() for k, v in enc.state_dict().items()}
    assert int(after["radar_bev_conv.1.bn.num_batches_tracked"]) == 8
    ev = encoder(R.SMALL, after, fused=False)
    assert torch.equal(out[:, 1:], ev([frames[1]]))
    twin = encoder(R.SMALL, sd, fused=False).train()
    twin.fused_grad = True
    assert torch.equal(out[:, 0], twin.extract_pts_feat(frames[0]))


def test_8_without_the_switch_training_mode_still_raises():
    enc = encoder(R.SMALL, R.make_state_dict(3)).train()
    assert type(enc).fused_grad is False and enc.fused_grad is False
    with pytest.raises(RuntimeError, match="training-mode BatchNorm"):
        enc.extract_pts_feat(clouds_b2())
    with pytest.raises(RuntimeError, match="training-mode BatchNorm"):
        enc([clouds_b2()])


def test_9_eval_mode_ignores_the_switch():
    sd, clouds = R.make_state_dict(3), clouds_b2()
    off = encoder(R.SMALL, sd)
    on = encoder(R.SMALL, sd)
    on.fused_grad = True
    a, b = off([clouds, clouds[::-1]]), on([clouds, clouds[::-1]])
    assert torch.equal(a, b) and not b.requires_grad
    assert torch.equal(off.extract_pts_feat(clouds), on.extract_pts_feat(clouds))


def test_10_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    p = ctypes.c_void_p(64)

    def refused(rc, text):
        assert rc == -1 and text in lib.rac_last_error(), lib.rac_last_error()

    refused(lib.rac_bn_train_stats_fwd(None, p, p, p, p, p, p, 2, 64, 16, 1e-5, 0.1, None), b"null pointer")
    refused(lib.rac_bn_train_stats_fwd(p, p, p, p, p, None, p, 2, 64, 16, 1e-5, 0.1, None), b"together")
    refused(lib.rac_bn_train_stats_fwd(p, p, p, p, p, p, p, 2, 96, 16, 1e-5, 0.1, None), b"multiple of 64")
    refused(lib.rac_bn_train_stats_fwd(p, p, p, p, p, p, p, 1, 64, 1, 1e-5, 0.1, None), b"at least 2")
    refused(lib.rac_bn_train_apply_fwd(p, p, p, None, p, p, 2, 64, 16, 1, None), b"null pointer")
    refused(lib.rac_bn_train_apply_fwd(p, p, p, p, p, p, 2, 32, 16, 1, None), b"multiple of 64")
    refused(lib.rac_bn_train_apply_fwd(p, p, p, p, p, p, 1, 64, 1, 1, None), b"at least 2")
    refused(lib.rac_bn_train_bwd(p, p, p, p, p, p, p, None, p, p, 2, 64, 16, None), b"null pointer")
    refused(lib.rac_bn_train_bwd(p, p, p, p, p, p, p, p, p, p, 2, 100, 16, None), b"multiple of 64")
    refused(lib.rac_bn_train_bwd(p, p, p, p, p, p, p, p, p, p, 1, 64, 1, None), b"at least 2")
    q = ctypes.c_void_p(128)
    refused(lib.rac_bn_train_bwd(p, q, None, p, p, p, p, p, p, q, 2, 64, 16, None), b"alias")
    geo = (0.8, 0.8, 8.0, -6.0, -6.0, -1.0, 16, 16, None)
    fwd = [p] * 16
    refused(lib.rac_pillar_train_fwd(*fwd[:3], None, *fwd[4:], 4, 1, 7, 10, 64, 1e-3, 0.01, *geo), b"null pointer")
    refused(lib.rac_pillar_train_fwd(None, *fwd[1:], 4, 1, 7, 10, 64, 1e-3, 0.01, *geo), b"null pointer")
    refused(lib.rac_pillar_train_fwd(*fwd, 4, 1, 7, 1, 64, 1e-3, 0.01, *geo), b"max_num_points")
    refused(lib.rac_pillar_train_fwd(*fwd, 4, 1, 7, 10, 32, 1e-3, 0.01, *geo), b"feature channels")
    refused(lib.rac_pillar_train_fwd(*fwd, 4, 1, 3, 10, 64, 1e-3, 0.01, *geo), b"point width")
    bwd = [p] * 14
    refused(lib.rac_pillar_train_bwd(None, *bwd[1:], 4, 1, 7, 10, 64, *geo), b"null pointer")
    refused(lib.rac_pillar_train_bwd(*bwd[:12], None, p, 4, 1, 7, 10, 64, *geo), b"null pointer")
    refused(lib.rac_pillar_train_bwd(*bwd, 4, 0, 7, 10, 64, *geo), b"n_clouds")
    refused(lib.rac_pillar_train_bwd(*bwd, 4, 1, 7, 40, 64, *geo), b"max_num_points")
