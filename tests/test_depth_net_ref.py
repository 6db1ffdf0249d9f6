"""DepthNet on the CPU (no GPU needed): the package's module and the functional restatement (tests/depth_net_ref.py) against the
REFERENCE's own class, recorded in tests/golden/depth_net_small{,.1}.npz by tests/golden/gen_golden_depth_net.py; the folded
weights and the lookup form of dep_proj that the HIP route uses, in float64; the argument checks of the new entry points.

Criterion for the reference's float32 run, as in tests/test_lss_view_ref.py: it may be 4 x E_ref from float64, E_ref = the float32
restatement's own error against the float64 one."""
import ctypes
import os

import numpy as np
import pytest
import torch

import depth_net_ref as R
from racformer_amd import depth_net as DN

MID, CONTEXT, D = 32, 16, 24


@pytest.fixture(scope="module")
def fixture(golden_dir):
    z = dict(np.load(os.path.join(golden_dir, "depth_net_small.npz")))
    z.update(np.load(os.path.join(golden_dir, "depth_net_small.1.npz")))
    sd = {k[3:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd:")}
    entries = {}
    for tag in ("a", "b"):
        e = {k[2:]: torch.from_numpy(v) for k, v in z.items() if k.startswith(tag + ":")}
        e["radar_feats"] = torch.nn.functional.one_hot(e["bins"].long(), D + 1).permute(0, 3, 1, 2).float().contiguous()
        e["rcs_embedding"] = e["rcs_table"][:, e["rcs_class"].long() + 1].permute(1, 0, 2, 3).contiguous()
        entries[tag] = e
    return sd, entries


def args(e, dtype=torch.float32):
    return [e[k].to(dtype) for k in ("x", "radar_feats", "rcs_embedding", "mlp_input")]


def module(sd, dtype=torch.float32, **kw):
    m = DN.DepthNet(MID, MID, CONTEXT, D, use_dcn=False, **kw).eval()
    m.load_state_dict(sd, strict=True)
    return m.to(dtype)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_reference_output_is_reproduced(fixture, tag):
    """strict load of the reference's state dict; the package's module and the restatement against the reference's output"""
    sd, entries = fixture
    e = entries[tag]
    assert tuple(e["x"].shape[2:]) == {"a": (16, 44), "b": (20, 23)}[tag] and int((e["bins"] == D).sum()) > 0 \
        and int((e["rcs_class"] == -1).sum()) > 0
    s64, e_ref = R.e_ref(sd, *args(e))
    assert e_ref["out"] > 0
    with torch.no_grad():
        got32, got64 = module(sd)(*args(e)), module(sd, torch.float64)(*args(e, torch.float64))
    err_ref = float((e["out"].double() - s64["out"]).abs().max())
    err_mod = float((got32.double() - s64["out"]).abs().max())
    print(f"{tag}: E_ref {e_ref['out']:.3g}, reference's float32 run {err_ref:.3g}, module's float32 run {err_mod:.3g}, "
          f"module float64 - restatement float64 {float((got64 - s64['out']).abs().max()):.3g}")
    assert e["out"].shape == s64["out"].shape == got32.shape
    assert err_ref <= 4 * e_ref["out"] and err_mod <= 4 * e_ref["out"]
    assert float((got64 - s64["out"]).abs().max()) <= 1e-12 * max(1.0, float(s64["out"].abs().max()))
    assert float((R.forward(sd, *args(e), torch.float32).double() - e["out"].double()).abs().max()) <= 8 * e_ref["out"]


def test_state_dict_keys_are_the_references(fixture):
    sd, _ = fixture
    m = DN.DepthNet(MID, MID, CONTEXT, D, use_dcn=False)
    assert sorted(m.state_dict()) == sorted(sd) and len(sd) == 106
    for key in ("reduce_conv.0.bias", "reduce_conv.1.running_var", "bn.running_mean", "depth_mlp.fc2.weight", "depth_se.conv_expand.bias",
                "dep_proj.weight", "depth_conv.2.bn2.weight", "depth_conv.3.aspp4.atrous_conv.weight", "depth_conv.3.global_avg_pool.2.bias",
                "depth_conv.3.conv1.weight", "depth_conv.3.bn1.running_mean", "depth_conv.4.bias", "context_conv.weight"):
        assert key in sd
    assert sorted(R.make_state_dict(MID, CONTEXT, D, 1)) == sorted(sd)
    assert all(R.make_state_dict(MID, CONTEXT, D, 1)[k].shape == v.shape for k, v in sd.items())


def test_variants_of_the_torch_route(fixture):
    """depth_only, the LayerNorm(9) variant of GN / SyncBN, use_aspp=False, other widths; use_dcn=True raises"""
    with pytest.raises(NotImplementedError, match="use_dcn=False"):
        DN.DepthNet(MID, MID, CONTEXT, D)
    with pytest.raises(NotImplementedError, match="use_dcn=False"):
        DN.DepthNet(MID, MID, CONTEXT, D, use_dcn=True)
    _, entries = fixture
    e = entries["b"]
    with torch.no_grad():
        only = DN.DepthNet(MID, MID, CONTEXT, D, use_dcn=False, depth_only=True).eval()
        assert not any(k.startswith("context_") for k in only.state_dict())
        assert only(*args(e)).shape == (2, D, 20, 23)
        gn = DN.DepthNet(MID, 48, CONTEXT, D, use_dcn=False, norm_cfg=dict(type='GN', num_groups=4)).eval()
        assert isinstance(gn.bn, torch.nn.LayerNorm) and isinstance(gn.reduce_conv[1], torch.nn.GroupNorm)
        assert gn(*args(e)).shape == (2, D + CONTEXT, 20, 23)
        assert isinstance(DN.DepthNet(MID, MID, CONTEXT, D, use_dcn=False, norm_cfg=dict(type='SyncBN')).bn, torch.nn.LayerNorm)
        plain = DN.DepthNet(MID, MID, CONTEXT, D, use_dcn=False, use_aspp=False).eval()
        assert len(plain.depth_conv) == 4 and plain(*args(e)).shape == (2, D + CONTEXT, 20, 23)
    assert not only.hip_route(e["x"], e["mlp_input"])           # CPU tensors: never the HIP route


def test_train_mode_and_backward(fixture):
    sd, entries = fixture
    e = entries["b"]
    m = module(sd).train()
    x = e["x"].clone().requires_grad_(True)
    out = m(x, *args(e)[1:])
    out.square().mean().backward()
    assert x.grad is not None and float(x.grad.abs().sum()) > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    assert int(m.reduce_conv[1].num_batches_tracked) == int(sd["reduce_conv.1.num_batches_tracked"]) + 1    # batch statistics ran


def test_folded_weights_reproduce_the_module(fixture):
    """The operands of the HIP route (every BatchNorm folded in float64, weights packed [tap][Cin][Cout], the BatchNorm1d in
    fc1, the image-pool branch as a bias of conv1) evaluated with float64 torch ops against the unfolded float64 module."""
    sd, entries = fixture
    m = module(sd)
    pk = m.packed()
    assert m.packed() is pk                                     # cached per weight version
    e = entries["b"]
    s64 = R.stages(sd, *args(e), torch.float64)
    F = torch.nn.functional

    def conv(x, wp, bias, k=1, dil=1, cout=MID):
        w = wp.double()[:, :, :cout].reshape(k, k, wp.shape[1], cout).permute(3, 2, 0, 1)
        return F.conv2d(x, w, bias.double() if bias is not None else None, padding=dil if k == 3 else 0, dilation=dil)

    tol = lambda ref: 1e-6 * float(ref.abs().max())             # noqa: E731  (float32 storage of the folded weights)
    x0 = torch.relu(conv(e["x"].double(), *pk["reduce"], k=3))
    assert float((x0 - s64["x0"]).abs().max()) <= tol(s64["x0"])
    # gates: the packed parameter block, layer by layer
    g = pk["gates"].double()
    mlp = e["mlp_input"].double().reshape(-1, 9)
    for row, br in enumerate(("context", "depth")):
        p, off = g[row], 0

        def take(n_in, n_out):
            nonlocal off
            w = p[off:off + n_in * n_out].view(n_in, n_out)
            b = p[off + n_in * n_out:off + n_in * n_out + n_out]
            off += n_in * n_out + n_out
            return w, b
        (w1, b1), (w2, b2), (wr, br_), (we, be) = take(9, MID), take(MID, MID), take(MID, MID), take(MID, MID)
        assert off == p.numel()
        gate = torch.sigmoid(torch.relu((torch.relu(mlp @ w1 + b1) @ w2 + b2) @ wr + br_) @ we + be)
        assert float((gate - s64[f"gate_{br}"]).abs().max()) <= 1e-6
    t = s64["b2"]
    cat = torch.cat([torch.relu(conv(t, w, b, k, dil)) for w, b, k, dil in pk["aspp"]], dim=1)
    wp, bp = pk["pool"]
    wc, bc, wb = pk["conv1"]
    img_bias = torch.relu(t.mean(dim=(2, 3)) @ wp.double() + bp.double()) @ wb.double()
    aspp = torch.relu(conv(cat, wc, bc) + img_bias[..., None, None])
    assert float((aspp - s64["aspp"]).abs().max()) <= tol(s64["aspp"])
    w1, b1, w2, b2 = pk["blocks"][0]
    blk = torch.relu(conv(torch.relu(conv(s64["dep"], w1, b1, 3)), w2, b2, 3) + s64["dep"])
    assert float((blk - s64["b0"]).abs().max()) <= tol(s64["b0"])
    assert float((conv(s64["aspp"], *pk["final"], cout=D) - s64["depth"]).abs().max()) <= tol(s64["depth"])
    # a changed weight is repacked
    with torch.no_grad():
        m.depth_conv[4].bias.add_(1.0)
    assert m.packed() is not pk and float((m.packed()["final"][1] - pk["final"][1] - 1).abs().max()) < 1e-6


def test_dep_proj_lookup_equals_the_dense_concatenation():
    """float64: gated features + one-hot grid + embedding through the dense 1x1 == the 1x1 over the features + one column per
    depth bin + one table row per RCS class -- with a pixel without radar return (bin D) and a pixel of class -1; and the
    module's own tables are those."""
    sd = R.make_state_dict(MID, CONTEXT, D, 5)
    inp = R.make_inputs(2, MID, D, 5, 7, 6)
    bins, cls, ew, eb = inp["bins"], inp["rcs_class"], inp["rcs_weight"].double(), inp["rcs_bias"].double()
    assert int(bins[0, 0, 0]) == D and int(cls[0, 0, 0]) == -1 and int((cls >= 0).sum()) > 0 and int((bins < D).sum()) > 0
    grid, emb = R.dense_priors(bins, cls, ew, eb, D)
    assert float(grid[0, :D, 0, 0].abs().sum()) == 0 and float(grid[0, D, 0, 0]) == 1            # "no return" is the last channel
    assert float((emb[0, :, 0, 0] - eb).abs().max()) == 0                                        # class -1: the bias alone
    gated = inp["x"].double() * torch.rand(2, MID, 1, 1, dtype=torch.float64)
    dense = torch.nn.functional.conv2d(torch.cat((gated, grid, emb), 1), sd["dep_proj.weight"].double(), sd["dep_proj.bias"].double())
    look = R.dep_proj_lookup(sd, gated, bins, cls, ew, eb, D)
    assert float((dense - look).abs().max()) <= 1e-13 * float(dense.abs().max())
    m = DN.DepthNet(MID, MID, CONTEXT, D, use_dcn=False).eval()
    m.load_state_dict(sd, strict=True)
    pk, table = m.packed(), m.rcs_table(inp["rcs_weight"], inp["rcs_bias"])
    w = sd["dep_proj.weight"].double()[:, :, 0, 0]
    mine = torch.nn.functional.conv2d(gated, w[:, :MID, None, None], sd["dep_proj.bias"].double()) \
        + pk["bins_table"].double()[bins.long()].permute(0, 3, 1, 2) + table.double()[cls.long() + 1].permute(0, 3, 1, 2)
    assert float((mine - dense).abs().max()) <= 1e-6 * float(dense.abs().max())                  # (tables stored in float32)
    assert m.rcs_table(inp["rcs_weight"], inp["rcs_bias"]) is table


def test_from_config_builds_the_references_depth_net():
    from racformer_amd import lss_depth as LD
    grid = dict(x=[-51.2, 51.2, 6.4], y=[-51.2, 51.2, 6.4], z=[-5.0, 3.0, 8.0], depth=[1.0, 65.0, 24.0], rcs=[-64, 64, 64])
    m = LD.LSSViewTransformerBEVDepth_racformer.from_config(grid_config=grid, input_size=(64, 96), downsample=16, in_channels=48,
                                                            out_channels=20, depthnet_cfg=dict(use_dcn=False))
    net = m.depth_net
    assert isinstance(net, DN.DepthNet) and (net.in_channels, net.mid_channels, net.context_channels, net.depth_channels) == (48, 48, 20, 24)
    assert "depth_net.depth_conv.3.aspp2.atrous_conv.weight" in m.state_dict()
    with pytest.raises(NotImplementedError):
        LD.LSSViewTransformerBEVDepth_racformer.from_config(grid_config=grid, input_size=(64, 96), downsample=16)
    with pytest.raises(TypeError):
        LD.LSSViewTransformerBEVDepth_racformer(grid_config=grid, input_size=(64, 96), downsample=16)


def test_argument_errors_need_no_gpu():
    """Every new entry point rejects bad arguments before any HIP call."""
    from racformer_amd import _lib
    lib = _lib.lib()
    one = ctypes.c_void_p(256)

    def desc(**kw):
        d = _lib.ConvSmall()
        d.in_, d.w, d.out = 256, 256, 256
        d.BN, d.H, d.W, d.Cin, d.Cout, d.ksize, d.dilation = 1, 4, 4, 32, 64, 3, 1
        d.ld_in, d.ld_w, d.ld_out = 32, 64, 64
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def conv_err(**kw):
        rc = lib.rac_conv_small_fwd(ctypes.byref(desc(**kw)), None)
        return rc, lib.rac_last_error()

    assert lib.rac_conv_small_fwd(None, None) == -1 and b"null descriptor" in lib.rac_last_error()
    for bad, text in ((dict(in_=None), b"null pointer"), (dict(w=None), b"null pointer"), (dict(out=None), b"null pointer"),
                      (dict(dilation=0), b"dilation=0"), (dict(ksize=2), b"ksize=2"), (dict(Cin=48), b"Cin=48"), (dict(Cin=0), b"Cin=0"),
                      (dict(ld_w=96), b"weight rows"), (dict(Cout=65), b"weight rows"), (dict(ld_in=16), b"input rows"),
                      (dict(in_=260), b"input rows"), (dict(gate=256, gate_channels=48), b"gate_channels=48"),
                      (dict(gate=256, gate_channels=64), b"gate_channels=64"), (dict(residual=256, ld_res=8), b"residual rows"),
                      (dict(bins=256), b"bins without a table"), (dict(cls=256), b"cls without a table"), (dict(out_layout=2), b"out_layout=2"),
                      (dict(c_off=1), b"do not fit"), (dict(H=0), b"H=0"), (dict(BN=-1), b"BN=-1")):
        rc, msg = conv_err(**bad)
        assert rc == -1 and text in msg, (bad, msg)
    assert lib.rac_conv_small_pack_fwd(None, one, 1, 4, 4, 8, 0, 0, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_conv_small_pack_fwd(one, one, 1, 4, 4, 8, 4, 1, None) == -1 and b"do not fit" in lib.rac_last_error()
    assert lib.rac_conv_small_pack_fwd(one, one, 1, 0, 4, 8, 0, 0, None) == -1
    assert lib.rac_depthnet_gates_fwd(one, None, one, 1, 256, 2, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_depthnet_gates_fwd(one, one, one, 1, 2048, 2, None) == -1 and b"C=2048" in lib.rac_last_error()
    assert lib.rac_depthnet_gates_fwd(one, one, one, 1, 256, 0, None) == -1
    assert lib.rac_depthnet_pool_bias_fwd(one, one, one, one, None, 1, 4, 256, 256, 256, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_depthnet_pool_bias_fwd(one, one, one, one, one, 1, 4, 128, 256, 256, None) == -1 and b"ld=128" in lib.rac_last_error()
    assert lib.rac_depthnet_pool_bias_fwd(one, one, one, one, one, 1, 0, 256, 256, 256, None) == -1
    # empty batches launch nothing and succeed
    assert lib.rac_conv_small_fwd(ctypes.byref(desc(BN=0)), None) == 0
