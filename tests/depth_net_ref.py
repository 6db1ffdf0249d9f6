"""DepthNet (models/necks/view_transformer_racformer.py:329-567 of the reference, use_dcn=False) restated functionally on a
state dict, in any dtype: ``F.conv2d`` / ``F.batch_norm`` on the reference's keys, and a second form with every BatchNorm folded
into its neighbour.  Shares no code with racformer_amd/depth_net.py.  The oracle of the CPU and GPU tests, and the source of
E_ref, the float32 restatement's own error (tests/radar_pillars_ref.py:175)."""
import math

import torch
import torch.nn.functional as F

EPS = 1e-5
DILATIONS = (1, 6, 12, 18)


def make_state_dict(mid, context, D, seed, n_emb=32):
    """A full state dict with the reference's keys: kaiming-normal convolutions, default-style Linear weights, and BatchNorm
    statistics and affine parameters away from their initial values."""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(name, co, ci, k, bias):
        sd[name + ".weight"] = torch.randn(co, ci, k, k, generator=g) * math.sqrt(2.0 / (ci * k * k))
        if bias:
            sd[name + ".bias"] = (torch.rand(co, generator=g) - 0.5) * 0.2

    def bn(name, c):
        sd[name + ".weight"] = 0.6 + 0.8 * torch.rand(c, generator=g)
        sd[name + ".bias"] = 0.2 * torch.randn(c, generator=g)
        sd[name + ".running_mean"] = 0.2 * torch.randn(c, generator=g)
        sd[name + ".running_var"] = 0.5 + torch.rand(c, generator=g)
        sd[name + ".num_batches_tracked"] = torch.tensor(7)

    def linear(name, co, ci):
        sd[name + ".weight"] = (torch.rand(co, ci, generator=g) - 0.5) * 2 / math.sqrt(ci)
        sd[name + ".bias"] = (torch.rand(co, generator=g) - 0.5) * 0.2

    conv("reduce_conv.0", mid, mid, 3, True)
    bn("reduce_conv.1", mid)
    conv("context_conv", context, mid, 1, True)
    bn("bn", 9)
    for br in ("depth", "context"):
        linear(f"{br}_mlp.fc1", mid, 9)
        linear(f"{br}_mlp.fc2", mid, mid)
        conv(f"{br}_se.conv_reduce", mid, mid, 1, True)
        conv(f"{br}_se.conv_expand", mid, mid, 1, True)
    conv("dep_proj", mid, mid + D + 1 + n_emb, 1, True)
    for i in range(3):
        conv(f"depth_conv.{i}.conv1", mid, mid, 3, False)
        bn(f"depth_conv.{i}.bn1", mid)
        conv(f"depth_conv.{i}.conv2", mid, mid, 3, False)
        bn(f"depth_conv.{i}.bn2", mid)
    for i, k in enumerate((1, 3, 3, 3)):
        conv(f"depth_conv.3.aspp{i + 1}.atrous_conv", mid, mid, k, False)
        bn(f"depth_conv.3.aspp{i + 1}.bn", mid)
    conv("depth_conv.3.global_avg_pool.1", mid, mid, 1, False)
    bn("depth_conv.3.global_avg_pool.2", mid)
    conv("depth_conv.3.conv1", mid, 5 * mid, 1, False)
    bn("depth_conv.3.bn1", mid)
    conv("depth_conv.4", D, mid, 1, True)
    return sd


def make_inputs(bn_maps, mid, D, h, w, seed, n_emb=32, n_rcs=64):
    """x, the index maps (a pixel without radar return = bin D, a pixel of RCS class -1 among them), the embedding parameters,
    the dense priors built from them, mlp_input [1, bn_maps, 9]."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(bn_maps, mid, h, w, generator=g)
    bins = torch.randint(0, D + 1, (bn_maps, h, w), generator=g, dtype=torch.int32)
    bins[torch.rand(bn_maps, h, w, generator=g) < 0.5] = D
    cls = torch.randint(-1, n_rcs, (bn_maps, h, w), generator=g, dtype=torch.int32)
    bins[0, 0, 0], cls[0, 0, 0] = D, -1
    bins[0, -1, -1], cls[0, -1, -1] = 0, n_rcs - 1
    ew = torch.randn(n_emb, n_rcs, 1, 1, generator=g) * 0.3
    eb = torch.randn(n_emb, generator=g) * 0.1
    mlp = torch.randn(1, bn_maps, 9, generator=g)
    return dict(x=x, bins=bins, rcs_class=cls, rcs_weight=ew, rcs_bias=eb, mlp_input=mlp)


def dense_priors(bins, cls, ew, eb, D):
    """(radar_feats [BN, D+1, h, w] one-hot, rcs_embedding [BN, E, h, w]) from the definitions (:688-693)"""
    grid = F.one_hot(bins.long(), D + 1).permute(0, 3, 1, 2).to(ew.dtype)
    one_hot = F.one_hot(cls.long() + 1, ew.shape[1] + 1)[..., 1:].permute(0, 3, 1, 2).to(ew.dtype)
    return grid, F.conv2d(one_hot, ew, eb)


def _cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def _bn(sd, name, x):
    return F.batch_norm(x, sd[name + ".running_mean"], sd[name + ".running_var"], sd[name + ".weight"], sd[name + ".bias"], False, 0.0, EPS)


def _folded(sd, conv, bn):
    """weight * g, (bias - mean) * g + beta in the state dict's dtype"""
    g = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + EPS)
    b = sd.get(conv + ".bias", torch.zeros_like(g))
    return sd[conv + ".weight"] * g.view(-1, 1, 1, 1), (b - sd[bn + ".running_mean"]) * g + sd[bn + ".bias"]


def _conv_bn(sd, conv, bn, x, folded, **kw):
    if folded:
        w, b = _folded(sd, conv, bn)
        return F.conv2d(x, w, b, **kw)
    return _bn(sd, bn, F.conv2d(x, sd[conv + ".weight"], sd.get(conv + ".bias"), **kw))


def gates(sd, mlp_input, branch, folded=False):
    """[BN, mid]: the sigmoid gate of the SE layer of ``branch`` ('depth' / 'context')"""
    m = mlp_input.reshape(-1, 9)
    if folded:
        g = sd["bn.weight"] / torch.sqrt(sd["bn.running_var"] + EPS)
        s = sd["bn.bias"] - sd["bn.running_mean"] * g
        h = F.linear(m, sd[f"{branch}_mlp.fc1.weight"] * g, sd[f"{branch}_mlp.fc1.weight"] @ s + sd[f"{branch}_mlp.fc1.bias"])
    else:
        h = F.linear(_bn(sd, "bn", m), sd[f"{branch}_mlp.fc1.weight"], sd[f"{branch}_mlp.fc1.bias"])
    h = F.linear(torch.relu(h), sd[f"{branch}_mlp.fc2.weight"], sd[f"{branch}_mlp.fc2.bias"])[..., None, None]
    h = torch.relu(F.conv2d(h, sd[f"{branch}_se.conv_reduce.weight"], sd[f"{branch}_se.conv_reduce.bias"]))
    return torch.sigmoid(F.conv2d(h, sd[f"{branch}_se.conv_expand.weight"], sd[f"{branch}_se.conv_expand.bias"]))[:, :, 0, 0]


def basic_block(sd, p, x, folded=False):
    out = torch.relu(_conv_bn(sd, p + ".conv1", p + ".bn1", x, folded, padding=1))
    return torch.relu(_conv_bn(sd, p + ".conv2", p + ".bn2", out, folded, padding=1) + x)


def pool_vector(sd, x, folded=False, p="depth_conv.3"):
    """[BN, mid, 1, 1]: ASPP's image-pool branch before the (constant) interpolation"""
    return torch.relu(_conv_bn(sd, p + ".global_avg_pool.1", p + ".global_avg_pool.2", x.mean(dim=(2, 3), keepdim=True), folded))


def aspp(sd, x, folded=False, p="depth_conv.3"):
    outs = []
    for i, d in enumerate(DILATIONS):
        kw = dict(padding=d, dilation=d) if i else {}
        outs.append(torch.relu(_conv_bn(sd, f"{p}.aspp{i + 1}.atrous_conv", f"{p}.aspp{i + 1}.bn", x, folded, **kw)))
    x5 = F.interpolate(pool_vector(sd, x, folded, p), size=x.shape[2:], mode="bilinear", align_corners=True)
    return torch.relu(_conv_bn(sd, p + ".conv1", p + ".bn1", torch.cat(outs + [x5], dim=1), folded))


def stages(sd, x, radar_feats, rcs_embedding, mlp_input, dtype, folded=False):
    """dict of every intermediate in ``dtype``: x0 (reduce_conv), gate_context, gate_depth, context, dep (dep_proj), b0..b2,
    aspp, depth, out"""
    sd = _cast(sd, dtype)
    x, radar_feats, rcs_embedding, mlp_input = (t.to(dtype) for t in (x, radar_feats, rcs_embedding, mlp_input))
    s = {}
    s["x0"] = torch.relu(_conv_bn(sd, "reduce_conv.0", "reduce_conv.1", x, folded, padding=1))
    s["gate_context"], s["gate_depth"] = gates(sd, mlp_input, "context", folded), gates(sd, mlp_input, "depth", folded)
    s["context"] = F.conv2d(s["x0"] * s["gate_context"][..., None, None], sd["context_conv.weight"], sd["context_conv.bias"])
    cat = torch.cat((s["x0"] * s["gate_depth"][..., None, None], radar_feats, rcs_embedding), dim=1)
    t = s["dep"] = F.conv2d(cat, sd["dep_proj.weight"], sd["dep_proj.bias"])
    for i in range(3):
        t = s[f"b{i}"] = basic_block(sd, f"depth_conv.{i}", t, folded)
    s["aspp"] = aspp(sd, t, folded)
    s["depth"] = F.conv2d(s["aspp"], sd["depth_conv.4.weight"], sd["depth_conv.4.bias"])
    s["out"] = torch.cat((s["depth"], s["context"]), dim=1)
    return s


def forward(sd, x, radar_feats, rcs_embedding, mlp_input, dtype, folded=False):
    return stages(sd, x, radar_feats, rcs_embedding, mlp_input, dtype, folded)["out"]


def dep_proj_lookup(sd, gated_x, bins, cls, ew, eb, D):
    """dep_proj in its lookup form: the 1x1 over the gated features + one column of the weight per depth bin + one row of
    W_r (E[:, class] + b_E) per RCS class (W_r b_E for class -1), in the inputs' dtype."""
    w = sd["dep_proj.weight"].to(gated_x.dtype)[:, :, 0, 0]
    mid = gated_x.shape[1]
    out = F.conv2d(gated_x, w[:, :mid, None, None], sd["dep_proj.bias"].to(gated_x.dtype))
    out = out + w[:, mid:mid + D + 1][:, bins.long()].permute(1, 0, 2, 3)
    e = ew.to(gated_x.dtype).reshape(ew.shape[0], -1)
    cols = torch.cat((torch.zeros_like(e[:, :1]), e), dim=1) + eb.to(gated_x.dtype).view(-1, 1)
    table = w[:, mid + D + 1:] @ cols                                   # [mid, n_rcs + 1]
    return out + table[:, (cls.long() + 1)].permute(1, 0, 2, 3)


def e_ref(sd, x, radar_feats, rcs_embedding, mlp_input):
    """(float64 stages, {stage: E_ref}): per stage the largest of |f32 unfolded - f64|, |f32 folded - f64|, |f32 folded - f32
    unfolded| (the definition of tests/radar_pillars_ref.py:175)"""
    s64 = stages(sd, x, radar_feats, rcs_embedding, mlp_input, torch.float64)
    a = stages(sd, x, radar_feats, rcs_embedding, mlp_input, torch.float32)
    b = stages(sd, x, radar_feats, rcs_embedding, mlp_input, torch.float32, folded=True)
    return s64, {k: three_way(a[k], b[k], s64[k]) for k in s64}


def three_way(a32, b32, r64):
    a, b = a32.double(), b32.double()
    return max(float((a - r64).abs().max()), float((b - r64).abs().max()), float((b - a).abs().max()))


def conv_layer(sd, conv, bn, x, dtype, folded, residual=None, relu=True, **kw):
    """One convolution layer on given inputs (teacher forcing): conv (+ BN if ``bn``) (+ residual) (+ ReLU) in ``dtype``"""
    sd = _cast(sd, dtype)
    x = x.to(dtype)
    y = _conv_bn(sd, conv, bn, x, folded, **kw) if bn else F.conv2d(x, sd[conv + ".weight"], sd.get(conv + ".bias"), **kw)
    if residual is not None:
        y = y + residual.to(dtype)
    return torch.relu(y) if relu else y


def conv_layer_e_ref(sd, conv, bn, x, **kw):
    r64 = conv_layer(sd, conv, bn, x, torch.float64, False, **kw)
    return r64, three_way(conv_layer(sd, conv, bn, x, torch.float32, False, **kw), conv_layer(sd, conv, bn, x, torch.float32, True, **kw), r64)
