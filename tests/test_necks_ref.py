"""The image necks without a GPU: torch routes of racformer_amd.necks against the reference's golden (tests/golden/necks_small.npz)
and the float64 restatement (tests/necks_ref.py), their state-dict keys, the refused configurations, the nearest-neighbour source
rule, and the argument errors of the two entry points."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import necks_ref as NR
from racformer_amd import necks
from racformer_amd.fpn_writer import FPNOutputWriter


def shapes_of(m):
    return {k: tuple(v.shape) for k, v in m.state_dict().items()}


def lss_case(golden_dir):
    g = np.load(os.path.join(golden_dir, "necks_small.npz"))
    m = necks.CustomFPN(NR.LSS["channels"], 256, num_outs=1, start_level=0, out_ids=[0]).eval()
    sd = NR.fill_state(shapes_of(m), int(g["lss:weight_seed"]))
    m.load_state_dict(sd)
    return g, m, sd, [torch.from_numpy(g["lss:in0"]), torch.from_numpy(g["lss:in1"])]


def fpn_case(golden_dir):
    g = np.load(os.path.join(golden_dir, "necks_small.npz"))
    m = necks.FPN(NR.FPN4["channels"], 256, 4).eval()
    sd = NR.fill_state(shapes_of(m), int(g["fpn:weight_seed"]))
    m.load_state_dict(sd)
    xs = NR.make_inputs(int(g["fpn:input_seed"]), NR.FPN4["images"], NR.FPN4["channels"], NR.FPN4["maps"], relu=True)
    return g, m, sd, xs


def test_custom_fpn_torch_route_vs_golden_and_float64(golden_dir):
    g, m, sd, xs = lss_case(golden_dir)
    assert sorted(sd) == list(g["lss:state_keys"])
    with torch.no_grad():
        got = m(xs)
    assert got.shape == (2, 256, 7, 11) and got.is_contiguous()
    # the reference ran the same fp32 torch ops: equal up to the order of its in-place add
    assert (got - torch.from_numpy(g["lss:out"])).abs().max().item() < 2e-6 * float(np.abs(g["lss:out"]).max())
    want = NR.custom_fpn(sd, xs)
    assert (got.double() - want).abs().max().item() < 1e-5 * float(want.abs().max())
    # the golden itself against float64: the restatement describes the reference
    assert (torch.from_numpy(g["lss:out"]).double() - want).abs().max().item() < 1e-5 * float(want.abs().max())


def test_fpn_torch_route_vs_golden_and_float64(golden_dir):
    g, m, sd, xs = fpn_case(golden_dir)
    assert sorted(sd) == list(g["fpn:state_keys"])
    ch = [int(c) for c in g["fpn:channels"]]
    assert ch == NR.FPN4_CHANNELS
    with torch.no_grad():
        got = m(xs)
    want = NR.fpn(sd, xs)
    assert isinstance(got, tuple) and len(got) == 4
    for i, (a, w) in enumerate(zip(got, want)):
        assert tuple(a.shape) == (6, 256) + tuple(NR.FPN4["maps"][i]) and a.is_contiguous()
        ref = torch.from_numpy(g[f"fpn:out{i}"])
        assert (a[:, ch] - ref).abs().max().item() < 2e-6 * float(ref.abs().max()), i
        assert (a.double() - w).abs().max().item() < 1e-5 * float(w.abs().max()), i
        assert (ref.double() - w[:, ch]).abs().max().item() < 1e-5 * float(w.abs().max()), i


def test_state_dict_keys():
    m = necks.FPN([256, 512, 1024, 2048], 256, 4)
    want = [f"{part}.{i}.conv.{p}" for part in ("lateral_convs", "fpn_convs") for i in range(4) for p in ("weight", "bias")]
    assert sorted(m.state_dict()) == sorted(want)
    assert m.lateral_convs[3].conv.weight.shape == (256, 2048, 1, 1) and m.fpn_convs[0].conv.weight.shape == (256, 256, 3, 3)
    c = necks.CustomFPN([1024, 2048], 256, num_outs=1, start_level=0, out_ids=[0])
    want = [f"lateral_convs.{i}.conv.{p}" for i in range(2) for p in ("weight", "bias")] + ["fpn_convs.0.conv.weight", "fpn_convs.0.conv.bias"]
    assert sorted(c.state_dict()) == sorted(want)


def test_fpn_takes_an_fpn_output_writer_state_dict():
    wr = FPNOutputWriter(num_levels=4, num_cams=6)
    m = necks.FPN([32, 64, 96, 128], 256, 4)
    res = m.load_state_dict(wr.state_dict(), strict=False)
    assert not res.unexpected_keys and all(k.startswith("lateral_convs.") for k in res.missing_keys)
    assert sorted(wr.state_dict()) == sorted(k for k in m.state_dict() if k.startswith("fpn_convs."))
    for k, v in wr.state_dict().items():
        assert torch.equal(m.state_dict()[k], v)


@pytest.mark.parametrize("kw", [dict(num_outs=5), dict(num_outs=3), dict(add_extra_convs=True), dict(add_extra_convs="on_input"),
                                dict(start_level=1), dict(end_level=3), dict(norm_cfg=dict(type="BN")), dict(act_cfg=dict(type="ReLU")),
                                dict(conv_cfg=dict(type="Conv2d")), dict(upsample_cfg=dict(mode="bilinear")),
                                dict(upsample_cfg=dict(scale_factor=2, mode="nearest")), dict(relu_before_extra_convs=True)])
def test_fpn_refuses_what_f8_does_not_use(kw):
    args = dict(in_channels=[32, 64, 96, 128], out_channels=256, num_outs=4)
    args.update(kw)
    with pytest.raises(NotImplementedError):
        necks.FPN(**args)


@pytest.mark.parametrize("kw", [dict(start_level=1), dict(end_level=2), dict(out_ids=[0, 1]), dict(out_ids=[1]), dict(out_ids=[]),
                                dict(num_outs=2), dict(add_extra_convs=True), dict(norm_cfg=dict(type="BN")),
                                dict(act_cfg=dict(type="ReLU")), dict(conv_cfg=dict(type="Conv2d")),
                                dict(upsample_cfg=dict(mode="bilinear")), dict(upsample_cfg=dict(scale_factor=2, mode="nearest"))])
def test_custom_fpn_refuses_what_is_not_configured(kw):
    args = dict(in_channels=[64, 128], out_channels=256, num_outs=1, start_level=0, out_ids=[0])
    args.update(kw)
    with pytest.raises(NotImplementedError):
        necks.CustomFPN(**args)


def test_forward_pregrouped_needs_the_hip_route():
    m = necks.FPN([32, 64], 256, 2).eval()
    with pytest.raises(RuntimeError), torch.no_grad():
        m.forward_pregrouped([torch.zeros(6, 32, 4, 4), torch.zeros(6, 64, 2, 2)])


def test_nearest_source_rule_is_torchs_exhaustively():
    """The host restatements of src(p) (racformer_amd.necks.nearest_src, what rac_fpn_lateral_fwd computes per axis; tests/necks_ref.py
    nearest_index) against F.interpolate(..., mode='nearest') for every 1 <= in <= 96, in <= out <= 2 in + 1."""
    for n_in in range(1, 97):
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
        for n_out in range(n_in, 2 * n_in + 2):
            want = F.interpolate(src, size=(n_out, 1), mode="nearest").view(-1).long().tolist()
            assert [necks.nearest_src(d, n_in, n_out) for d in range(n_out)] == want, (n_in, n_out)
            assert [NR.nearest_index(d, n_in, n_out) for d in range(n_out)] == want, (n_in, n_out)
            # and along the other axis (torch's kernels take the two axes through the same function)
        want_w = F.interpolate(src.view(1, 1, 1, n_in), size=(1, 2 * n_in - 1), mode="nearest").view(-1).long().tolist()
        assert [necks.nearest_src(d, n_in, 2 * n_in - 1) for d in range(2 * n_in - 1)] == want_w


def test_upsample_restatement_matches_interpolate():
    t = torch.randn(2, 3, 4, 6, dtype=torch.float64)
    for size in [(7, 11), (8, 12), (4, 6), (5, 6)]:
        assert torch.equal(NR.upsample_nearest(t, size), F.interpolate(t, size=size, mode="nearest"))


def test_entry_point_argument_errors_need_no_gpu():
    """Argument validation of rac_fpn_lateral_fwd and rac_conv3x3_cf_fwd happens before any HIP call."""
    from racformer_amd import _lib
    lib = _lib.lib()
    p16 = ctypes.c_void_p(16)

    def lateral(x=p16, w=p16, bias=None, top=None, out=p16, N=1, Cin=64, H=4, W=6, th=0, tw=0, Cout=256):
        return lib.rac_fpn_lateral_fwd(x, w, 1.0, bias, top, out, N, Cin, H, W, th, tw, Cout, None)

    for kw, msg in [(dict(x=None), b"null pointer"), (dict(w=None), b"null pointer"), (dict(out=None), b"null pointer"),
                    (dict(Cin=48), b"multiple of 32"), (dict(Cin=0), b"multiple of 32"), (dict(Cout=128), b"256 output channels"),
                    (dict(H=0), b"H=0"), (dict(top=p16, th=5, tw=6), b"no larger than the output"),
                    (dict(top=p16, th=4, tw=7), b"no larger than the output"), (dict(top=p16, th=0, tw=3), b"at least 1x1"),
                    (dict(w=ctypes.c_void_p(8)), b"16-byte aligned"), (dict(bias=ctypes.c_void_p(24)), b"16-byte aligned")]:
        assert lateral(**kw) == -1, kw
        assert msg in lib.rac_last_error(), (kw, lib.rac_last_error())
    assert lateral(x=None, w=None, out=None, N=0) == 0

    def conv(xs=p16, ws=p16, bias=None, amax=p16, out=p16, N=1, H=4, W=6, Cin=256, Cout=256):
        return lib.rac_conv3x3_cf_fwd(xs, ws, bias, amax, 1.0, out, N, H, W, Cin, Cout, None)

    for kw, msg in [(dict(xs=None), b"null pointer"), (dict(ws=None), b"null pointer"), (dict(amax=None), b"null pointer"),
                    (dict(out=None), b"null pointer"), (dict(Cin=40), b"multiple of 32"), (dict(Cout=64), b"256 output channels"),
                    (dict(W=0), b"W=0"), (dict(bias=ctypes.c_void_p(8)), b"16-byte aligned")]:
        assert conv(**kw) == -1, kw
        assert msg in lib.rac_last_error(), (kw, lib.rac_last_error())
    assert conv(xs=None, ws=None, amax=None, out=None, N=0) == 0
