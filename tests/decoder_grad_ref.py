"""What the generator of tests/golden/decoder_grad_small.npz and the tests that read it share: the tiny rig, the seeded,
name-keyed weights (float16-exact; a function of the seed, not stored: the layer has 14 M parameters), the seeded inputs, the
discrete choices float32 and float64 must agree on, how a large gradient is sampled, and the error metric.

Rig: one decoder layer, Q = 21, 2 cameras (front and back), T = 2, 4 pyramid levels as in racsampling_grad_small
(4x12, 2x6, 1x3, 1x2; image 64 x 176), num_points 2 x depth 3 for the image sampling, 2 x 5 for the BEV sampling, BEV maps 16 x 16,
layer index 1 (d_region 0.1), num_ray 150, B = 1."""
import zlib

import numpy as np
import torch

import bev_sampling_ref as BR
import sampling4d_core_ref as SR
from racformer_amd import synthetic as syn
from racformer_amd.transformer import box_table_torch

E, G, T, NP, D, Q, N = 256, 4, 2, 2, 3, 21, 2
NP_BEV, D_BEV, HEADS = 2, 5, 4
IMG_HW, HWS, BEV_HW = (64, 176), [(4, 12), (2, 6), (1, 3), (1, 2)], (16, 16)
LAYER, NUM_RAY = 1, 150
D_REGION_LIST = [0.15, 0.1, 0.1, 0.08, 0.08, 0.05]
D_REGION = D_REGION_LIST[LAYER]
WEIGHT_SEED = 7
SAMPLE = 1024            # entries kept of a gradient with more than FULL elements
FULL = 2048
LAYER_KW = dict(embed_dims=E, num_frames=T, num_points=NP, num_points_bev=NP_BEV, num_levels=len(HWS), num_classes=10, code_size=10,
                img_depth_num=D, bev_depth_num=D_BEV, num_ray=NUM_RAY, pc_range=list(syn.PC_RANGE), d_region_list=D_REGION_LIST,
                spatial_shapes=BEV_HW)


def make_weights(shapes, seed=WEIGHT_SEED):
    """name -> float32 array, float16-exact, drawn name-keyed from PCG64: weights N(0, 1 / fan_in), LayerNorm gains 1 + N(0, 0.1^2),
    biases N(0, 0.05^2), embeddings N(0, 0.5^2), the two kinds of sampling offsets' biases U(-1.5, 1.5)"""
    w = {}
    for k, shp in shapes.items():
        rng = np.random.default_rng((seed * 7919 + zlib.crc32(k.encode())) & 0x7FFFFFFF)
        shp = tuple(shp)
        if "embed" in k:
            a = rng.standard_normal(shp, dtype=np.float32) * np.float32(0.5)
        elif k.endswith("sampling_offset.bias"):
            a = rng.uniform(-1.5, 1.5, shp).astype(np.float32)
        elif len(shp) == 1 and k.endswith(".weight"):
            a = 1 + rng.standard_normal(shp, dtype=np.float32) * np.float32(0.1)
        elif len(shp) == 1:
            a = rng.standard_normal(shp, dtype=np.float32) * np.float32(0.05)
        else:
            a = rng.standard_normal(shp, dtype=np.float32) * np.float32(1.0 / np.sqrt(np.prod(shp[1:])))
        w[k] = a.astype(np.float16).astype(np.float32)
    return w


def draw(seed):
    """the inputs of one layer call and the gouts of (query_feat, cls_score, bbox_xy)"""
    rng = np.random.default_rng(seed)
    qr = rng.random((1, Q, 10), dtype=np.float32)
    qr[..., 1] = 0.15 + 0.5 * qr[..., 1]
    qr[:, -2:, 1] = np.float32(0.93)                      # near the rim: keypoints beyond the map, clamped
    qr[:, -2, 0], qr[:, -1, 0] = np.float32(0.02), np.float32(0.27)
    qr[..., 2] = 0.1 + 0.8 * qr[..., 2]
    qr[..., 6:8] = qr[..., 6:8] * 2 - 1
    qr[..., 8:10] = qr[..., 8:10] * 4 - 2
    d = dict(query_bbox=qr, query_feat=rng.standard_normal((1, Q, E), dtype=np.float32))
    for i, (h, w) in enumerate(HWS):                     # channel-last [S,N,H,W,64], multiples of 1/8
        d[f"feat{i}"] = np.round(rng.standard_normal((T * G, N, h, w, 64), dtype=np.float32) * 8) / np.float32(8)
    for k in ("lss", "radar"):
        d[k] = np.round(rng.standard_normal((1, T, E, *BEV_HW), dtype=np.float32) * 8) / np.float32(8)
    d["time_diff"] = np.arange(T, dtype=np.float32)[None] * np.float32(0.5) + rng.random((1, T), dtype=np.float32) * np.float32(0.1)
    d["lidar2img"] = np.stack(syn.ring_lidar2img(T, N, IMG_HW))[None].astype(np.float32)
    d.update(gout_feat=rng.standard_normal((1, Q, E), dtype=np.float32), gout_cls=rng.standard_normal((1, Q, 10), dtype=np.float32),
             gout_xy=rng.standard_normal((1, Q, 10), dtype=np.float32))
    return d


def discrete_steps(w, d, x1, pred, dtype):
    """every discrete choice of the layer, evaluated in ``dtype`` from that precision's own norm1 output ``x1`` and refined boxes
    ``pred``: image sampling -- camera, clamp gates, homo gate, any-valid, the tap cell of every level --; both BEV samplings --
    clamp gates and the tap cell --; the refinement -- the clamp gates of inverse_sigmoid and of theta_d2xy_coods"""
    t = lambda a: torch.as_tensor(np.asarray(a)).to(dtype)  # noqa: E731
    x, qb, td = x1.detach().to(dtype), t(d["query_bbox"]), t(d["time_diff"])
    lin = lambda k: x @ t(w[k + ".weight"]).t() + t(w[k + ".bias"])  # noqa: E731
    box = box_table_torch(qb, syn.PC_RANGE)
    c = SR.chain64(box, qb[..., 8:10], lin("sampling.sampling_offset"), lin("sampling.ray_points_offset"), td, t(d["lidar2img"]),
                   G, NP, D, syn.PC_RANGE, D_REGION, IMG_HW[0], IMG_HW[1])
    res = [c["view"], (c["ux"] >= 0) & (c["ux"] <= 1), (c["uy"] >= 0) & (c["uy"] <= 1), c["homo"] > 1e-5, c["any_valid"],
           SR.floors(c["u"], c["v"], HWS)]
    for m in ("sampling_radar_bev", "sampling_lss_bev"):
        loc = BR.chain64(box[0], qb[0, :, 8:10], lin(m + ".sampling_offset")[0], lin(m + ".ray_points_offset")[0], td[0], HEADS, NP_BEV,
                         D_BEV, syn.PC_RANGE, D_REGION, clamp=False, dtype=dtype)
        res += [(loc >= 0) & (loc <= 1)]
        cl = loc.clamp(0, 1)
        res += [torch.floor(cl[..., 0] * BEV_HW[1] - 0.5).long(), torch.floor(cl[..., 1] * BEV_HW[0] - 0.5).long()]
    p, o = qb[..., 1:3], pred.detach().to(dtype)
    res += [p >= 0, p <= 1, p >= 1e-5, 1 - p >= 1e-5]
    ang, rad = o[..., 0] * (2 * np.pi), o[..., 1] * 65.0
    for u in ((51.2 + rad * torch.cos(ang)) / 102.4, (51.2 + rad * torch.sin(ang)) / 102.4):
        res += [u >= 0, u <= 1]
    return res


def same_choices(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def sample_index(name, numel):
    """the entries of a gradient the fixture keeps: all of them up to FULL elements, else SAMPLE name-keyed random positions"""
    if numel <= FULL:
        return None
    return np.sort(np.random.default_rng(zlib.crc32(name.encode())).choice(numel, SAMPLE, replace=False))


def sampled(name, a):
    a = np.asarray(a).reshape(-1)
    idx = sample_index(name, a.size)
    return a if idx is None else a[idx]


def rel_err(got, want64, scale):
    """max |got - f64| over the kept entries / max |f64| over the WHOLE tensor (stored as ``scale``)"""
    return float(np.abs(np.asarray(got, dtype=np.float64) - np.asarray(want64, dtype=np.float64)).max() / scale)


def bound(ref_figure):
    """per tensor: twice the reference's own float32-against-float64 figure (another, equally rounded summation order), and
    never below 1e-5 of the largest element, the bound of the module fixtures"""
    return max(2 * float(ref_figure), 1e-5)


def grads_of(layer, leaves):
    """name -> gradient (numpy) of every parameter of ``layer`` ("p:<name>") and every input leaf"""
    g = {"p:" + k: p.grad.detach().cpu().numpy() for k, p in layer.named_parameters()}
    g.update({k: v.grad.detach().cpu().numpy() for k, v in leaves.items()})
    return g


# ------------------------------------------------------------------------------------------------ reading the fixture
def load_golden(golden_dir):
    import os
    g = {}
    for name in ("decoder_grad_small.npz", "decoder_grad_small.1.npz"):
        with np.load(os.path.join(golden_dir, name)) as z:
            g.update({k: z[k] for k in z.files})
    return g


def build_layer(g, device="cpu", dtype=torch.float32):
    """the package's decoder layer with the fixture's weights (regenerated from the stored seed, checked against the stored sums)"""
    from racformer_amd.transformer import RaCFormerTransformerDecoderLayer
    layer = RaCFormerTransformerDecoderLayer(**LAYER_KW).eval()
    w = make_weights({k: v.shape for k, v in layer.state_dict().items()}, int(g["weight_seed"]))
    assert sorted(w) == [str(k) for k in g["weight_names"]], "state_dict keys differ from the reference's"
    assert np.array_equal(np.array([w[k].astype(np.float64).sum() for k in sorted(w)]), g["weight_sums"]), "weights differ from the generator's"
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return layer.to(device=device, dtype=dtype)


def run_layer(layer, g, device="cpu", dtype=torch.float32):
    """one call of the layer under autograd on the fixture's inputs, the fixture's gouts backpropagated -> (outputs, gradients by
    fixture name, every one as numpy)"""
    t = lambda k: torch.from_numpy(np.asarray(g[k]).astype(np.float32)).to(device=device, dtype=dtype)  # noqa: E731
    leaves = {k: t(k).requires_grad_() for k in ("query_bbox", "query_feat", "lss", "radar")}
    leaves.update({f"feat{i}": t(f"feat{i}").requires_grad_() for i in range(len(HWS))})
    metas = [dict(img_shape=[(IMG_HW[0], IMG_HW[1], 3)], time_diff=t("time_diff"), lidar2img=t("lidar2img"))]
    td_safe = t("time_diff").clone()
    td_safe[td_safe < 1e-5] = 1.0
    metas[0]["time_diff_safe"] = td_safe
    layer.zero_grad(set_to_none=True)
    layer._carry = None
    feat, cls, pred = layer(leaves["query_bbox"], leaves["query_feat"], [leaves[f"feat{i}"] for i in range(len(HWS))], leaves["lss"],
                            leaves["radar"], None, metas, layer=LAYER)
    xy = layer.last_bbox_xy
    ((feat * t("gout_feat")).sum() + (cls * t("gout_cls")).sum() + (xy * t("gout_xy")).sum()).backward()
    out = dict(out_feat=feat, out_cls=cls, out_pred=pred, out_xy=xy)
    return {k: v.detach().cpu().numpy() for k, v in out.items()}, grads_of(layer, leaves)


def check_against_golden(g, out, grads, what, report=None):
    """outputs within 1e-5 of the largest element of the float64 reference; per gradient tensor, the error against the stored
    float64 gradient (kept entries) over max |f64| (whole tensor) <= bound(the reference's own figure).  -> the failures"""
    names = sorted(k[4:] for k in g if k.startswith("g64:"))
    assert sorted(grads) == names, f"{what}: gradient tensors {sorted(set(grads) ^ set(names))} do not pair up with the fixture"
    bad = []
    for k, v in out.items():
        want = g["out64_" + k[4:]]
        e = rel_err(v, want, float(np.abs(want).max()))
        if e > 1e-5:
            bad.append(f"{k}: {e:.2e} > 1e-5")
    for k in names:
        e = rel_err(sampled(k, grads[k]), g["g64:" + k], float(g["max64:" + k]))
        b = bound(g["ref:" + k])
        if report is not None:
            report.append((k, e, float(g["ref:" + k]), b))
        if not e <= b:
            bad.append(f"{k}: {e:.2e} > max(2 x {float(g['ref:' + k]):.2e}, 1e-5)")
    return bad
