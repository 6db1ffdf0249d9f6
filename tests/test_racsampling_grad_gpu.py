"""rac_sampling4d_bwd on the MI355X: the backward of the fused adaptive 4D sampling kernel, stage by stage.

  1  the keypoints the backward recomputes (u, v, camera, level weights) are the forward's loc_out / w_out bit for bit;
  2  the gather half (grad_loc_out, grad_w_out, grad_feats) against float64 evaluated at the kernel's own float32 locations and
     cameras, and against rac_msmv_bwd_ex at those locations;
  3  the chain tail and the sums (grad_offsets, grad_ray, grad_scale, grad_box) element by element against the float64 closed
     form fed the kernel's own per-keypoint gradients and cameras, with a negative control (a reference without the clamp gates
     must fail the same check).  The clamp and homo > eps gates of that reference come from its float64 chain; the test asserts
     that no keypoint lies within 1e-5 of a gate, a hundred float32 roundings;
  4  the module against the reference's own autograd (tests/golden/racsampling_grad_small.npz), 5e-6 / 1e-5 of the largest
     element as for bev_sampling_grad_small;
  5  at the f8 shape: the grad-mode forward is the no_grad forward bit for bit, and every module gradient (query_ray, query_feat,
     the four levels, the six Linear parameters) against float64 with the kernel's own cameras imposed through force_views: the
     closed form of sampling4d_core_ref (shown on the CPU to be float64 autograd of the torch chain + gather) run in float64 on
     the device from the float32 Linear outputs the kernel read, gathered at the kernel's loc_out so that every floor is the
     kernel's, then the Linears and the box table backwards in float64;
  6  two runs: everything but grad_feats bitwise equal, grad_feats within 1e-5 of its largest element.

Metric: worst |err| / A in units of 2^-24, A the same sum with every term non-negative (sampling4d_core_ref, magnitude=True).
For query_ray at f8 A is the largest of the query's row: box_table_torch's Jacobian has entries that cancel to zero in float64
(the cosine of a quarter turn) where float32 leaves 4e-8, so an element's own A can be 1e-17 of its row's.

Measured on an MI355X (worst over the five shapes; the bounds are the next power of two above the kernel's figure):
  stages 2 and 3, K = 32:  grad_u 0.77, grad_v 0.39, grad_wl 0.94, grad_feats 6.44 (against rac_msmv_bwd_ex 0.61, 0.38, 1.05,
      6.63); tail: grad_offsets 23.44, grad_ray 6.62, grad_scale 7.72, grad_box 13.98;
  f8 module gradients, the same K: feature levels 6.27, scale_weights.weight 0.38, every other parameter and query_feat < 0.05;
  end to end against float64 at float64's OWN locations, kernel | torch's float32 autograd of the route the module had before
  (torch keypoint chain + sampling_4d / rac_msmv_bwd_ex, the kernel's cameras imposed), per shape l4, p1_l2_oddGT, p128, 3cam, l1:
      offsets  31.0|29.2   17.7|21.5   33.1|32.5    43.5|73.5    23.9|46.0
      ray      0.35|0.20   0.22|0.39   0.13|0.08    0.30|1.30    1.60|1.15
      scale    47.5|63.6   30.9|42.7   55.8|40.8   116.8|100.9    0|0
      query    2.99|3.02   6.74|19.1   0.75|0.83   10.1|11.9     7.71|8.44
      feats    4.4e5|5.7e5  3.3e4|4.9e4  4.0e3|4.1e3  3.7e4|5.3e4  8.5e3|5.2e3
  asserted per shape and kind: kernel <= 2 x torch, and kernel <= K_E2E = 128 for all kinds but feats.  The feats figures of
  both routes are the float32 rounding of the location itself (a tap weight moves by (W-1) times it, and a pixel that only a
  vanishing tap reaches has an A as small), which stage 2 takes out by evaluating float64 at the kernel's locations."""
import numpy as np
import pytest
import torch

import sampling4d_core_ref as SR
import test_racsampling_grad_cpu as TC
from racformer_amd import synthetic as syn
from racformer_amd import transformer as T
from racformer_amd.fused import sampling4d_backward, sampling4d_fused
from racformer_amd.msmv import msmv_backward

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K = 32.0
K_E2E = 128.0
IMG = (64, 176)

#          Q  G  T  NP D  N  levels                              outside three_cam
SHAPES = [(9, 4, 2, 2, 3, 6, [(8, 22), (4, 11), (2, 6), (1, 3)], True, False),
          (7, 3, 3, 1, 1, 6, [(8, 22), (4, 11)], False, False),                    # P = 1, odd G*T: quirk Q1 is not the identity
          (5, 1, 2, 32, 4, 6, [(8, 22), (4, 11), (2, 6), (1, 3)], True, False),    # P = 128, the limit
          (8, 4, 2, 4, 3, 3, [(8, 22), (4, 11), (2, 6), (1, 3)], True, True),      # 3-camera rig (the compact forward)
          (6, 2, 2, 2, 2, 6, [(8, 22)], False, False)]                             # L = 1
IDS = ["l4", "p1_l2_oddGT", "p128", "3cam", "l1"]


def run_case(shape, view_in=None, want_feats=True):
    Q, G, Tn, NP, D, N, hws, outside, three_cam = shape
    c, gout = TC._case(Q + G + Tn + N + len(hws), Q, G, Tn, NP, D, N, hws, outside, three_cam)
    dev = {k: ([f.float().to(DEV) for f in v] if k == "feats" else v.float().to(DEV)) for k, v in c.items() if k in
           ("feats", "query_bbox", "off", "ray", "sc", "td", "l2i")}
    gout_d = gout.float().to(DEV)
    c = {**c, **{k: ([f.cpu().double() for f in v] if k == "feats" else v.cpu().double()) for k, v in dev.items()}}   # the float32 values
    args = (dev["feats"], dev["query_bbox"], dev["off"], dev["ray"], dev["sc"], dev["td"], dev["l2i"])
    cfg = (Tn, G, NP, D, c["pc"], c["d_region"], IMG[0], IMG[1])
    fwd = None
    if len(hws) != 1:          # (the forward kernel has no single-level instantiation)
        fwd = sampling4d_fused(*args, *cfg, debug=True, view_in=view_in)
    bwd = sampling4d_backward(*args, gout_d, *cfg, view_in=view_in, want_feats=want_feats, debug=True)
    torch.cuda.synchronize()
    return c, gout_d.cpu().double(), dev, fwd, bwd


def kernel_views(loc, N):
    return torch.round(loc[..., 2] * max(N - 1, 1)).to(torch.uint8).contiguous()


@pytest.mark.parametrize("shape", SHAPES[:4], ids=IDS[:4])
def test_recomputed_keypoints_are_the_forwards_bits(shape):
    _, _, _, fwd, bwd = run_case(shape)
    assert torch.equal(fwd[1], bwd[7]) and torch.equal(fwd[2], bwd[8])
    # with imposed cameras as well (loc_out then reports the kernel's own choice beside the imposed view's u, v)
    N = shape[5]
    vin = ((kernel_views(fwd[1], N).long() + 1) % N).to(torch.uint8).contiguous()
    _, _, _, fwd2, bwd2 = run_case(shape, view_in=vin)
    assert torch.equal(fwd2[1], bwd2[7]) and torch.equal(fwd2[2], bwd2[8]) and not torch.equal(fwd2[1], fwd[1])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gather_half_and_chain_tail_against_float64(shape):
    Q, G, Tn, NP, D, N, hws, outside, three_cam = shape
    c, gout, dev, fwd, bwd = run_case(shape)
    gfeats, goff, gray, gsc, gbox, gloc, gw, loc, w = (([f.cpu() for f in x] if isinstance(x, list) else x.cpu()) for x in bwd)
    B = 1
    views = kernel_views(loc, N)
    at = (loc[..., 0], loc[..., 1])
    kw = dict(view_in=views, loc_at=at, f32_coords=True)
    want = SR.closed_form_bwd(gout=gout, **c, **kw)
    mag = SR.closed_form_bwd(gout=gout, magnitude=True, **c, **kw)
    fig = {}
    # 2: the gather half at the kernel's own locations
    for name, got, key in (("grad_u", gloc[..., 0], "grad_u"), ("grad_v", gloc[..., 1], "grad_v"), ("grad_wl", gw, "grad_wl")):
        fig[name] = SR.metric(SR.from_slots(got, B, Tn, G), want[key], mag[key])
    for l in range(len(hws)):
        fig[f"grad_feat{l}"] = SR.metric(gfeats[l], want["grad_feats"][l], mag["grad_feats"][l])
    # ... and against rac_msmv_bwd_ex there (its own level weights: the kernel's)
    gf2, gloc2, gw2 = msmv_backward(dev_gout(gout), dev["feats"], bwd[7].contiguous(), bwd[8].contiguous(), grad_layout=1, num_frames=Tn,
                                    num_groups=G)
    torch.cuda.synchronize()
    fig["msmv:grad_u"] = SR.metric(SR.from_slots(gloc[..., 0], B, Tn, G), SR.from_slots(gloc2[..., 0].cpu(), B, Tn, G), mag["grad_u"])
    fig["msmv:grad_v"] = SR.metric(SR.from_slots(gloc[..., 1], B, Tn, G), SR.from_slots(gloc2[..., 1].cpu(), B, Tn, G), mag["grad_v"])
    fig["msmv:grad_wl"] = SR.metric(SR.from_slots(gw, B, Tn, G), SR.from_slots(gw2.cpu(), B, Tn, G), mag["grad_wl"])
    for l in range(len(hws)):
        fig[f"msmv:grad_feat{l}"] = SR.metric(gfeats[l], gf2[l].cpu(), mag["grad_feats"][l])
    # 3: the chain tail and the sums, fed the kernel's own per-keypoint gradients
    given = tuple(SR.from_slots(x.double(), B, Tn, G) for x in (gloc[..., 0], gloc[..., 1], gw))
    tail = SR.closed_form_bwd(gout=gout, given=given, **c, **kw)
    tmag = SR.closed_form_bwd(gout=gout, given=given, magnitude=True, **c, **kw)
    got = dict(grad_offsets=goff, grad_ray=gray, grad_scale=gsc, grad_box=gbox)
    for k in got:
        fig["tail:" + k] = SR.metric(got[k], tail[k], tmag[k])
    # (the float64 chain supplies the tail's clamp and homo > eps gates: no keypoint of these cases is within float32 rounding of one)
    assert SR.gate_margin(tail["chain"]) > 1e-5
    # end to end against float64 at float64's own locations (the kernel's cameras), and torch's float32 autograd of the route
    # the module had before (torch chain + sampling_4d) against the same: the kernel within 2x of it per gradient kind
    e2e = SR.closed_form_bwd(gout=gout, view_in=views, **c)
    emag = SR.closed_form_bwd(gout=gout, view_in=views, magnitude=True, **c)
    qw, qa = SR.box_to_query(c["query_bbox"], c["pc"], e2e["grad_box"]), SR.box_to_query(c["query_bbox"], c["pc"], emag["grad_box"], True)
    base = torch_route_grads(shape, c, dev, views.to(DEV), dev_gout(gout))
    qb_leaf = dev["query_bbox"].clone().requires_grad_()
    T.box_table_torch(qb_leaf, c["pc"]).backward(bwd[4])
    kern = dict(feats=gfeats, offsets=goff, ray=gray, scale=gsc, query=qb_leaf.grad.cpu())

    def kinds(g):
        r = {k: SR.metric(g[k], e2e["grad_" + k], emag["grad_" + k]) for k in ("offsets", "ray", "scale")}
        r["feats"] = max(SR.metric(g["feats"][l], e2e["grad_feats"][l], emag["grad_feats"][l]) for l in range(len(hws)))
        r["query"] = SR.metric(g["query"], qw, qa)
        return r
    ek, eb = kinds(kern), kinds(base)
    print("\n" + "\n".join(f"  {k:>24s}: {v:8.2f} x 2^-24" for k, v in fig.items()))
    print("\n".join(f"  {'e2e:' + k:>24s}: kernel {ek[k]:8.2f}   torch float32 route {eb[k]:8.2f}" for k in ek))
    bad = {k: v for k, v in fig.items() if not v <= K}
    assert not bad, bad
    bad = {k: (ek[k], eb[k]) for k in ek if not (ek[k] <= 2 * eb[k] and (k == "feats" or ek[k] <= K_E2E))}
    assert not bad, bad
    assert all(float(gbox[..., i].abs().max()) > 0 for i in range(8))
    if outside:      # negative control: a reference without the clamp gates must fail the same check
        wrong = SR.closed_form_bwd(gout=gout, given=given, wrong_term=True, **c, **kw)
        assert SR.metric(goff, wrong["grad_offsets"], tmag["grad_offsets"]) > K


def torch_route_grads(shape, c, dev, views, gout):
    """float32 autograd of the unfused route on the case's inputs, the kernel's cameras imposed -> the five gradient kinds (CPU)"""
    Q, G, Tn, NP, D, N, hws, _, _ = shape
    lv = {k: dev[k].clone().requires_grad_() for k in ("query_bbox", "off", "ray", "sc")}
    fs = [f.clone().requires_grad_() for f in dev["feats"]]
    out = SR.torch_route(lv["query_bbox"], lv["off"], lv["ray"], lv["sc"], fs, dev["td"], dev["l2i"], Tn, G, NP, D, len(hws),
                         c["pc"], c["d_region"], IMG[0], IMG[1], view_in=views)
    out.backward(gout)
    torch.cuda.synchronize()
    return dict(feats=[f.grad.cpu() for f in fs], offsets=lv["off"].grad.cpu(), ray=lv["ray"].grad.cpu(), scale=lv["sc"].grad.cpu(),
                query=lv["query_bbox"].grad.cpu())


def dev_gout(gout):
    return gout.float().to(DEV).contiguous()


def test_module_against_the_reference_golden(golden_dir):
    g = TC.load_golden(golden_dir)
    m = TC.module_from(g).to(DEV)
    qr, qf, feats, metas, gout = TC.inputs_from(g, device=DEV)
    out = m(qr, qf, feats, metas, d_region=float(g["d_region"]))
    assert out.grad_fn is not None
    (out * gout).sum().backward()
    torch.cuda.synchronize()
    TC.check_against_golden(g, m, qr, qf, feats, out, tol_out=5e-6, tol_grad=1e-5)


def test_f8_module_gradients_against_float64_and_two_runs_agree():
    from oracle import restate as R
    cfg = syn.F8
    tr = T.RaCFormerTransformer(**cfg.transformer_kwargs()).eval()
    syn.fill_params(tr, 22)
    tr = tr.to(DEV)
    qb, qf = syn.make_queries(cfg, 21)
    qf = qf * 5.0
    metas = syn.make_img_metas(cfg)
    tr.decoder.stage_metas(metas, cfg.batch, torch.device(DEV))
    smp = tr.decoder.decoder_layer.sampling
    feats = [f.to(DEV).requires_grad_() for f in R.regroup_pyramid(syn.make_pyramid(cfg, 21), cfg.num_cams)]
    qb, qf = qb.to(DEV).requires_grad_(), qf.to(DEV).requires_grad_()
    d_region = cfg.d_region_list[2]
    Tn, G, NP, D, N, L = cfg.num_frames, cfg.num_groups, cfg.num_points, cfg.img_depth_num, cfg.num_cams, cfg.num_levels
    with torch.no_grad():
        plain, loc, _ = smp(qb, qf, feats, metas, d_region=d_region, debug=True)
        views = kernel_views(loc, N)
        smp.force_views = [views]
        forced = smp(qb, qf, feats, metas, d_region=d_region)
        lin = [x(qf) for x in (smp.sampling_offset, smp.ray_points_offset, smp.scale_weights)]
    gout = torch.randn(plain.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    runs = []
    for _ in range(2):
        for x in (qb, qf, *feats, *smp.parameters()):
            x.grad = None
        smp.force_views = [views]
        out = smp(qb, qf, feats, metas, d_region=d_region)
        assert out.grad_fn is not None and torch.equal(out, forced)
        (out * gout).sum().backward()
        torch.cuda.synchronize()
        runs.append(dict(query_ray=qb.grad.clone(), query_feat=qf.grad.clone(), **{f"feat{i}": f.grad.clone() for i, f in enumerate(feats)},
                         **{k: p.grad.clone() for k, p in smp.named_parameters()}))
    for k, a in runs[0].items():
        b = runs[1][k]
        assert bool(a.isfinite().all()) and float(a.abs().max()) > 0, k
        if k.startswith("feat"):
            assert float((a - b).abs().max()) <= 1e-5 * float(a.abs().max()), k
        else:
            assert torch.equal(a, b), k
    assert float(qb.grad[..., 8:].abs().max()) == 0.0
    # float64 (on the device): the closed form -- on the CPU shown to be float64 autograd of the torch chain + gather -- from
    # the float32 Linear outputs the kernel read, gathered at the kernel's own locations and cameras (so every floor is the
    # kernel's), then the three Linears and the box table backwards in float64
    c = dict(feats=[f.detach() for f in feats], query_bbox=qb.detach(), off=lin[0], ray=lin[1], sc=lin[2], td=metas[0]["time_diff"],
             l2i=metas[0]["lidar2img"], gout=gout, T=Tn, G=G, NP=NP, D=D, pc=smp.pc_range, d_region=d_region,
             image_h=cfg.image_hw[0], image_w=cfg.image_hw[1], view_in=views, loc_at=(loc[..., 0], loc[..., 1]), f32_coords=True)
    want, mag = SR.closed_form_bwd(**c), SR.closed_form_bwd(magnitude=True, **c)
    ref, scale = {}, {}
    for dst, r, ab in ((ref, want, lambda x: x), (scale, mag, torch.abs)):
        dst["query_ray"] = SR.box_to_query(qb, smp.pc_range, r["grad_box"], magnitude=r is mag)
        if r is mag:      # (the scale of a query's row: its largest entry, see the docstring)
            dst["query_ray"] = dst["query_ray"].amax(-1, keepdim=True).expand(-1, -1, 10).clone()
            dst["query_ray"][..., 8:] = 0
        x64, gq = ab(qf.detach().double()[0]), 0
        for name, key in (("sampling_offset", "grad_offsets"), ("ray_points_offset", "grad_ray"), ("scale_weights", "grad_scale")):
            gl = r[key][0]                                                 # [Q, width]
            dst[name + ".weight"], dst[name + ".bias"] = gl.T @ x64, gl.sum(0)
            gq = gq + gl @ ab(getattr(smp, name).weight.detach().double())
        dst["query_feat"] = gq[None]
        dst.update({f"feat{i}": g for i, g in enumerate(r["grad_feats"])})
    fig = {k: SR.metric(runs[0][k], ref[k], scale[k]) for k in runs[0]}
    print("\n" + "\n".join(f"  {k:>28s}: {v:8.2f} x 2^-24" for k, v in fig.items()))
    bad = {k: v for k, v in fig.items() if not v <= K}
    assert not bad, bad


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[3]], ids=["l4", "3cam"])
def test_two_runs_of_the_kernel(shape):
    _, _, _, _, a = run_case(shape)
    _, _, _, _, b = run_case(shape)
    for x, y in zip(a[1:], b[1:]):
        assert torch.equal(x, y)
    for x, y in zip(a[0], b[0]):
        assert float((x - y).abs().max()) <= 1e-5 * float(x.abs().max())
    # without a feature gradient wanted: the same everything else
    _, _, _, _, n = run_case(shape, want_feats=False)
    assert n[0] is None and all(torch.equal(x, y) for x, y in zip(a[1:], n[1:]))
