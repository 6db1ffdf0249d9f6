"""The radar pillar branch's training route on the GPU (``RadarPillarEncoder.fused_grad``; rac_bn_train_*, rac_pillar_train_*)
against the float64 restatement of tests/radar_pillars_grad_ref.py.

Criterion, per tensor: err < max(4 x E_ref, 1e-5 x max|want|), E_ref the float32 CPU run of the same computation against float64, with
the GPU's decisions (ReLU masks, winning slots) imposed on both for every gradient.  Forward tensors are compared with float64's OWN
decisions; where the GPU decided otherwise, the float64 pre-activation has to lie within the stage's forward allowance of zero (for a
slot: the two candidates' float64 values within twice that allowance of each other) -- no count is capped."""
import numpy as np
import pytest
import torch
import torch.nn as nn

import radar_pillars_grad_ref as G
import radar_pillars_ref as R
from racformer_amd import radar_pillars as RP
from racformer_amd import resnet
from racformer_amd import synthetic as syn
from test_radar_pillars_ref import encoder, hand_points

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RAGGED = dict(R.SMALL, point_cloud_range=[-8.0, -4.8, -5.0, 8.0, 4.8, 3.0])          # a 12 x 20 map


def train_encoder(cfg, sd):
    enc = encoder(cfg, sd).to(DEV).train()
    enc.fused_grad = True
    return enc


def rn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def flips_within(what, own, gpu, pre64, allow):
    """decisions that differ from float64's own sit at pre-activations within the forward allowance of zero"""
    diff = own != gpu
    worst = float(pre64[diff].abs().max()) if bool(diff.any()) else 0.0
    print(f"\n{what}: {int(diff.sum())} ReLU decisions differ from float64's, largest |pre-activation| {worst:.3e}, allowance {allow:.3e}")
    assert worst <= allow, f"{what}: a differing decision at pre-activation {worst:.3e}, allowance {allow:.3e}"


# ------------------------------------------------------------------------------------------------ 1. the BatchNorm kernels alone
BN_CASES = {
    "n2": ((1, 64, 1, 2), 0.0),
    "odd": ((3, 64, 11, 13), 0.0),
    "c256": ((2, 256, 16, 16), 0.0),
    "chunks4": ((1, 64, 128, 128), 0.0),
    "far_mean": ((3, 64, 11, 13), 1.0e3),          # channel means of about 1e3 x the channel's standard deviation
}


def test_1_chunk_geometry_of_the_cases():
    """one case does not fill a partial-sum chunk of the kernel as built, one spans several"""
    assert RP.bn_chunks(1, 2) == 1 and 1 * 2 < 4096
    assert RP.bn_chunks(3, 11 * 13) == 1
    assert RP.bn_chunks(1, 128 * 128) == 4


def _bn_state(c, seed):
    sd = {}
    full = R.make_state_dict(seed)
    for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked"):
        v = full["radar_bev_conv.2.bn." + n]
        sd[n] = v[:c].clone() if v.dim() else v.clone()
    return sd


def _bn_reference(sd, x, g, mask, dtype):
    c = x.shape[1]
    bn = nn.BatchNorm2d(c)
    bn.load_state_dict(sd)
    bn = bn.to(dtype).train()
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    pre = bn(xr)
    (pre * mask.to(dtype)).backward(g.to(dtype))
    xd = x.detach().to(dtype)
    mean, var = xd.mean(dim=(0, 2, 3)), xd.var(dim=(0, 2, 3), unbiased=False)
    return dict(mean=mean, invstd=torch.rsqrt(var + bn.eps), y=torch.relu(pre.detach()), pre=pre.detach(), dx=xr.grad, dgamma=bn.weight.grad,
                dbeta=bn.bias.grad, running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
                tracked=int(bn.num_batches_tracked))


@pytest.mark.parametrize("name", sorted(BN_CASES))
def test_1_batchnorm_kernels_against_float64(name):
    shape, far = BN_CASES[name]
    c = shape[1]
    x = rn(100 + len(name), *shape)
    if far:
        sign = torch.where(torch.arange(c) % 2 == 0, 1.0, -1.0).view(1, c, 1, 1)
        x = x * (0.5 + torch.rand(c, generator=torch.Generator().manual_seed(3)).view(1, c, 1, 1)) + far * sign
    g = rn(200 + len(name), *shape)
    sd = _bn_state(c, 21)
    bn = nn.BatchNorm2d(c)
    bn.load_state_dict(sd)
    bn = bn.to(DEV).train()
    xd, gd = x.to(DEV), g.to(DEV)
    mean, invstd = RP.bn_train_stats(xd, bn)
    y = RP.bn_train_apply(xd, mean, invstd, bn.weight, bn.bias)
    dgamma, dbeta, dx = RP.bn_train_bwd(gd, xd, y, mean, invstd, bn.weight)
    dgamma2, dbeta2, none = RP.bn_train_bwd(gd, xd, y, mean, invstd, bn.weight, need_dx=False)
    torch.cuda.synchronize()
    assert none is None and torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta)
    mask = (y > 0).cpu()
    w64, w32 = _bn_reference(sd, x, g, mask, torch.float64), _bn_reference(sd, x, g, mask, torch.float32)
    got = dict(mean=mean, invstd=invstd, y=y, dx=dx, dgamma=dgamma, dbeta=dbeta, running_mean=bn.running_mean, running_var=bn.running_var)
    flips_within(f"bn {name}", w64["pre"] > 0, mask, w64["pre"], G.bound(w64["y"], w32["y"])[0])
    for k, v in got.items():
        G.hold(f"bn {name} {k}", v, w64[k], w32[k])
    assert int(bn.num_batches_tracked) == w64["tracked"] == 8
    if far:
        # the case has teeth: sum x^2 / n - mean^2 in float32 misses the criterion on invstd
        x32 = x.float()
        naive = torch.rsqrt(((x32 * x32).mean(dim=(0, 2, 3)) - x32.mean(dim=(0, 2, 3)) ** 2).clamp_min(0) + bn.eps)
        assert float((naive.double() - w64["invstd"]).abs().max()) > G.bound(w64["invstd"], w32["invstd"])[0]


# ------------------------------------------------------------------------------------------------ 2. the PFN layer alone
def _shapes_cloud():
    """a pillar with exactly P = 10 points, one with a single point, one holding the same point three times"""
    g = np.random.default_rng(5)
    p = np.zeros((14, 7), np.float32)
    p[:10, :2] = np.asarray([0.1, 0.1], np.float32) + g.random((10, 2), dtype=np.float32) * 0.6          # cell (8, 8)
    p[10, :2] = [2.0, -3.0]
    p[11:14, :2] = [-4.5, 4.5]
    p[:, 3:] = g.standard_normal((14, 4)).astype(np.float32) * 3
    p[11:14] = p[11]
    return [torch.from_numpy(p)]


def _single_cloud():
    p = np.zeros((3, 7), np.float32)
    p[:, :2] = [[0.1, 0.2], [0.3, 0.5], [0.7, 0.1]]
    p[:, 3:] = np.arange(12, dtype=np.float32).reshape(3, 4) - 5
    return [torch.from_numpy(p)]


def _no_pillar_clouds():
    p = np.zeros((4, 7), np.float32)
    p[:, 0] = 100.0                                          # outside the range
    return [torch.from_numpy(p), torch.zeros(0, 7)]


PFN_RIGS = {
    "hand": (R.HAND, lambda: [torch.from_numpy(hand_points())]),
    "small_b2": (R.SMALL, lambda: syn.make_radar_points(2, [0, 300], seed=5, grid=16, edge_fraction=0.2)),
    "shapes": (R.SMALL, _shapes_cloud),
    "single": (R.SMALL, _single_cloud),
    "none": (R.SMALL, _no_pillar_clouds),
    "no_points": (R.SMALL, lambda: [torch.zeros(0, 7)]),
}
PFN_NAMES = G.PARAMS[:3]
PFN_BUFFERS = G.BUFFERS[:3]


def _pfn_gpu(enc, clouds):
    vl, pfn = enc.radar_voxel_layer, enc.radar_voxel_encoder
    gx, gy, _ = vl.geom.grid
    pts, off = RP.pack_clouds([c.to(DEV) for c in clouds], zero_z=True)
    pv = RP.voxelize_packed(pts, off, vl.geom, vl.max_num_points, vl.cap())
    canvas, saved = pfn.train_fwd(pv, gy, gx)
    return canvas, saved


@pytest.mark.parametrize("name", sorted(PFN_RIGS))
def test_2_pfn_layer_against_float64(name):
    cfg, make = PFN_RIGS[name]
    clouds = make()
    sd = R.make_state_dict(31)
    enc = train_encoder(cfg, sd)
    canvas, saved = _pfn_gpu(enc, clouds)
    gout = rn(41, *canvas.shape)
    dw, dgamma, dbeta = enc.radar_voxel_encoder.train_bwd(saved, gout.to(DEV))
    dw2, dgamma2, dbeta2 = enc.radar_voxel_encoder.train_bwd(saved, gout.to(DEV), need_dw=False)
    torch.cuda.synchronize()
    assert dw2 is None and torch.equal(dgamma2, dgamma) and torch.equal(dbeta2, dbeta)
    keep = (saved[1][:, 0] >= 0).cpu()
    slots, feats = saved[7].cpu()[keep].long(), saved[6].cpu()[keep]
    v, c, n = R.voxelize_batch(clouds, zero_z=True, **cfg)
    assert slots.shape == (v.shape[0], 64) and int(saved[5]) == v.shape[0] * cfg["max_num_points"]
    got_buf = {k: enc.state_dict()[k].cpu() for k in PFN_BUFFERS}
    if name in ("none", "no_points"):
        assert v.shape[0] == 0 and not bool(canvas.any())
        assert all(torch.equal(got_buf[k], sd[k]) for k in PFN_BUFFERS)                      # untouched
        assert not bool(dw.any()) and not bool(dgamma.any()) and not bool(dbeta.any())
        return
    if name == "shapes":
        assert sorted(n.tolist()) == [1, 3, 10]
    if name == "single":
        assert v.shape[0] == 1
    dec = dict(slots=slots, pos=feats > 0)
    res = {}
    for dtype in (torch.float64, torch.float32):
        ts = G.TrainStages(sd, dtype, cfg)
        f_own, own, win, pre = ts.pfn(v, c, n)
        own_canvas = ts.scatter(f_own, c, len(clouds)).detach()
        ts = G.TrainStages(sd, dtype, cfg)                              # (a fresh one: the step above moved its statistics)
        for k in PFN_NAMES:
            ts.tensor(k).requires_grad_(True)
        f_imp, _, _, _ = ts.pfn(v, c, n, **dec)
        ts.scatter(f_imp, c, len(clouds)).backward(gout.to(dtype))
        res[dtype] = dict(canvas=own_canvas, own=own, win=win.detach(), pre=pre.detach(), grads={k: ts.tensor(k).grad for k in PFN_NAMES},
                          buf={k: ts.tensor(k).detach().clone() for k in PFN_BUFFERS})
    w64, w32 = res[torch.float64], res[torch.float32]
    allow = G.bound(w64["canvas"], w32["canvas"])[0]
    G.hold(f"pfn {name} canvas", canvas, w64["canvas"], w32["canvas"])
    # slots: where the GPU's winner is not float64's, the two candidates' float64 values are within twice the allowance
    P = v.shape[1]
    y64 = torch.relu(w64["pre"])
    pick = lambda s: y64.gather(1, torch.where(s < 0, n.long().view(-1, 1).expand(-1, 64).clamp(max=P - 1), s).unsqueeze(1)).squeeze(1)  # noqa: E731
    differ = slots != w64["own"]
    gap = float((pick(slots) - pick(w64["own"]))[differ].abs().max()) if bool(differ.any()) else 0.0
    print(f"\npfn {name}: {int(differ.sum())} winning slots differ from float64's, largest gap {gap:.3e}, allowance {allow:.3e}")
    assert gap <= 2 * allow
    pre_gpu_winner = w64["pre"].gather(1, torch.where(slots < 0, n.long().view(-1, 1).expand(-1, 64).clamp(max=P - 1), slots).unsqueeze(1)).squeeze(1)
    flips_within(f"pfn {name}", pre_gpu_winner > 0, feats > 0, pre_gpu_winner, allow)
    for k, got in zip(PFN_NAMES, (dw, dgamma, dbeta)):
        G.hold(f"pfn {name} grad {k}", got, w64["grads"][k], w32["grads"][k])
    for k in PFN_BUFFERS[:2]:
        G.hold(f"pfn {name} {k}", got_buf[k], w64["buf"][k], w32["buf"][k])
    assert int(got_buf[PFN_BUFFERS[2]]) == int(w64["buf"][PFN_BUFFERS[2]]) == 8


# ------------------------------------------------------------------------------------------------ 3. one ConvModule, teacher-forced
@pytest.fixture(scope="module")
def stage_rigs():
    sd = R.make_state_dict(51)
    out = {}
    for name, cfg, clouds in (("16x16", R.SMALL, syn.make_radar_points(2, [40, 300], seed=3, grid=16, edge_fraction=0.2)),
                              ("12x20", RAGGED, syn.make_radar_points(2, [150, 60], seed=4, grid=12, edge_fraction=0.2))):
        enc = train_encoder(cfg, sd)
        pts, off = RP.pack_clouds([c.to(DEV) for c in clouds], zero_z=True)
        _, _, layers = enc.train_forward_hip(pts, off)
        torch.cuda.synchronize()
        out[name] = (cfg, enc, layers)
    return sd, out


@pytest.mark.parametrize("layer", [0, 2])
@pytest.mark.parametrize("name", ["16x16", "12x20"])
def test_3_conv_layer_teacher_forced(stage_rigs, name, layer):
    sd, rigs = stage_rigs
    cfg, enc, layers = rigs[name]
    x, z, y, mean, invstd = layers[layer]
    assert tuple(x.shape[2:]) == ((16, 16) if name == "16x16" else (12, 20))
    gout = rn(61 + layer, *y.shape)
    bn = enc.radar_bev_conv[layer].bn
    dgamma, dbeta, gz = RP.bn_train_bwd(gout.to(DEV), z, y, mean, invstd, bn.weight)
    dw, _ = resnet.conv_wgrad(gz, x, 3, 1, bias=False)
    dx = resnet.conv_dgrad(gz, enc.train_packs(layer, transposed=True), 3, 1, x.shape[2:])
    torch.cuda.synchronize()
    mask, names = (y > 0).cpu(), [f"radar_bev_conv.{layer}.{n}" for n in ("conv.weight", "bn.weight", "bn.bias")]
    res = {}
    for dtype in (torch.float64, torch.float32):
        ts = G.TrainStages(sd, dtype, cfg)
        own, pre = ts.conv_layer(layer, x.cpu())
        ts = G.TrainStages(sd, dtype, cfg)
        for k in names:
            ts.tensor(k).requires_grad_(True)
        xin = x.cpu().to(dtype).requires_grad_(True)
        ts.conv_layer(layer, xin, mask)[0].backward(gout.to(dtype))
        res[dtype] = dict(y=own.detach(), pre=pre.detach(), dx=xin.grad, grads=[ts.tensor(k).grad for k in names])
    w64, w32 = res[torch.float64], res[torch.float32]
    G.hold(f"layer {layer} {name} y", y, w64["y"], w32["y"])
    flips_within(f"layer {layer} {name}", w64["pre"] > 0, mask, w64["pre"], G.bound(w64["y"], w32["y"])[0])
    G.hold(f"layer {layer} {name} dx", dx, w64["dx"], w32["dx"])
    for k, got, a, b in zip(names, (dw, dgamma, dbeta), w64["grads"], w32["grads"]):
        G.hold(f"layer {layer} {name} {k}", got, a, b)


# ------------------------------------------------------------------------------------------------ 4 - 6. the route
def e2e_clouds():
    return syn.make_radar_points(2, [300, 120], seed=9, grid=16, edge_fraction=0.2)


def run_route(enc, clouds, gout, spy=None):
    """extract_pts_feat forward + backward -> (output, {parameter: grad}, {buffer: value})"""
    for p in enc.parameters():
        p.grad = None
    if spy is not None:
        orig = enc.train_forward_hip

        def wrapped(*a):
            spy["saved"] = orig(*a)
            return spy["saved"]
        enc.train_forward_hip = wrapped
    out = enc.extract_pts_feat([c.to(DEV) for c in clouds])
    out.backward(gout.to(DEV))
    torch.cuda.synchronize()
    if spy is not None:
        del enc.train_forward_hip
    named, state = dict(enc.named_parameters()), enc.state_dict()
    return out.detach(), {k: named[k].grad for k in G.PARAMS}, {k: state[k].clone() for k in G.BUFFERS}


@pytest.fixture(scope="module")
def e2e():
    sd, clouds = R.make_state_dict(71), e2e_clouds()
    gout = rn(72, 2, 256, 16, 16)
    enc = train_encoder(R.SMALL, sd)
    spy = {}
    out, grads, bufs = run_route(enc, clouds, gout, spy)
    return dict(sd=sd, clouds=clouds, gout=gout, out=out, grads=grads, bufs=bufs, saved=spy["saved"])


def test_4_end_to_end_against_float64(e2e):
    sd, clouds, gout = e2e["sd"], e2e["clouds"], e2e["gout"]
    _, pfn_saved, layers = e2e["saved"]
    keep = (pfn_saved[1][:, 0] >= 0).cpu()
    dec = dict(slots=pfn_saved[7].cpu()[keep].long(), pos=pfn_saved[6].cpu()[keep] > 0, masks=[(l[2] > 0).cpu() for l in layers])
    v, c, n = R.voxelize_batch(clouds, zero_z=True, **R.SMALL)
    assert e2e["out"].shape == (2, 256, 16, 16) and e2e["out"].dtype == torch.float32
    w64 = G.grads_and_buffers(sd, R.SMALL, torch.float64, v, c, n, 2, gout, dec)
    w32 = G.grads_and_buffers(sd, R.SMALL, torch.float32, v, c, n, 2, gout, dec)
    o64 = G.grads_and_buffers(sd, R.SMALL, torch.float64, v, c, n, 2, gout)           # float64's own decisions
    o32 = G.grads_and_buffers(sd, R.SMALL, torch.float32, v, c, n, 2, gout)
    G.hold("e2e output", e2e["out"], o64[0], o32[0])
    for i in range(3):
        allow = G.bound(o64[3]["layer_out"][i].detach(), o32[3]["layer_out"][i].detach())[0]
        pre = o64[3]["layer_pre"][i].detach()
        flips_within(f"e2e layer {i}", pre > 0, dec["masks"][i], pre, allow)
    for k in G.PARAMS:
        assert e2e["grads"][k] is not None, k
        G.hold(f"e2e grad {k}", e2e["grads"][k], w64[1][k], w32[1][k])
    for k in G.BUFFERS:
        if k.endswith("num_batches_tracked"):
            assert int(e2e["bufs"][k]) == int(w64[2][k]) == 8
        else:
            G.hold(f"e2e {k}", e2e["bufs"][k], w64[2][k], w32[2][k])


def test_4_two_runs_from_one_state_give_the_same_bits(e2e):
    enc = train_encoder(R.SMALL, e2e["sd"])
    out, grads, bufs = run_route(enc, e2e["clouds"], e2e["gout"])
    assert torch.equal(out, e2e["out"])
    assert all(torch.equal(grads[k], e2e["grads"][k]) for k in G.PARAMS)
    assert all(torch.equal(bufs[k], e2e["bufs"][k]) for k in G.BUFFERS)


def test_5_forward_over_two_frames_follows_the_reference(e2e):
    sd = e2e["sd"]
    clouds = syn.make_radar_points(4, [300, 120, 0, 200], seed=10, grid=16, edge_fraction=0.2)
    frames = [[clouds[0].to(DEV), clouds[1].to(DEV)], [clouds[2].to(DEV), clouds[3].to(DEV)]]
    enc = train_encoder(R.SMALL, sd)
    with torch.no_grad():
        enc.eval()
        enc(frames)                                           # fills the eval caches on the OLD statistics
        enc.train()
    out = enc(frames)
    assert out.shape == (2, 2, 256, 16, 16) and out.requires_grad and enc.training
    after = {k: v.clone() for k, v in enc.state_dict().items()}
    first = train_encoder(R.SMALL, sd).extract_pts_feat(frames[0])
    assert torch.equal(out[:, 0], first)
    ev = encoder(R.SMALL, {k: v.cpu() for k, v in after.items()}).to(DEV)
    with torch.no_grad():
        second = ev([frames[1]])
    assert torch.equal(out[:, 1:], second)                    # (fails on stale _folded / _packed caches)
    assert not torch.equal(second, encoder(R.SMALL, sd).to(DEV)([frames[1]]))
    # the training route once more with unchanged weights: forward + backward without a host synchronisation
    gout = e2e["gout"].to(DEV)
    enc.extract_pts_feat(frames[0]).backward(gout)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        enc.extract_pts_feat(frames[0]).backward(gout)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(enc.radar_bev_conv[0].bn.num_batches_tracked) == 7 + 3


def test_6_frozen_stages_skip_their_launches(e2e, monkeypatch):
    enc = train_encoder(R.SMALL, e2e["sd"])
    frozen = [k for k in G.PARAMS if k.startswith(("radar_voxel_encoder", "radar_bev_conv.0."))]
    for k, p in enc.named_parameters():
        p.requires_grad_(k not in frozen)
    calls = {"dgrad": 0, "pfn": 0}
    dgrad, pfn_bwd = resnet.conv_dgrad, RP.PillarFeatureNet.train_bwd
    monkeypatch.setattr(resnet, "conv_dgrad", lambda *a, **k: (calls.__setitem__("dgrad", calls["dgrad"] + 1), dgrad(*a, **k))[1])
    monkeypatch.setattr(RP.PillarFeatureNet, "train_bwd", lambda *a, **k: (calls.__setitem__("pfn", calls["pfn"] + 1), pfn_bwd(*a, **k))[1])
    out, grads, bufs = run_route(enc, e2e["clouds"], e2e["gout"])
    assert calls == {"dgrad": 1, "pfn": 0}                    # only layer 2 -> layer 1
    assert torch.equal(out, e2e["out"])
    for k in G.PARAMS:
        if k in frozen:
            assert grads[k] is None, k
        else:
            assert torch.equal(grads[k], e2e["grads"][k]), k
