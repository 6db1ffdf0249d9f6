"""The depth branch around DepthNet on the CPU: the restatement (tests/lss_depth_ref.py) and the CPU route of
racformer_amd/lss_depth.py against the reference's own run (tests/golden/lss_depth_small.npz, gen_golden_lss_depth.py), the
depth-bin edges against the numpy float32 yardstick, and the C-ABI's argument checks.  No GPU.

Bounds.  Index maps, pooled depths and one-hots: exact.  Loss and gradients: the same operations in another association (einsum
against multiply-and-sum, conv2d over a one-hot against a gather), so first-order rounding of a reordered sum of n terms,
n * 2^-24 * sum |terms|, with n = D + pixels for the loss and its gradient and n = pixels for the embedding's gradients."""
import ctypes

import numpy as np
import pytest
import torch

import lss_depth_ref as R
from racformer_amd import lss_depth as LD
from racformer_amd import synthetic as syn

U = 2.0 ** -24
TAGS = ("a", "b")
GRID_XYZ = dict(x=[-51.2, 51.2, 6.4], y=[-51.2, 51.2, 6.4], z=[-5.0, 3.0, 8.0])


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return {t: R.golden(golden_dir, t) for t in TAGS + ("edges",)}


def maps(fx, key):
    t = torch.from_numpy(fx[key])
    return t.view(-1, *t.shape[-2:])


def module_for(fx, out_channels=8, in_channels=16, mid=12, **kw):
    grid = dict(GRID_XYZ, **R.golden_grid(fx))
    D = int(grid["depth"][2])
    H, W = fx["radar_depth"].shape[-2:]
    net = R.StandInDepthNet(in_channels, D + 1 + 32, mid, D + out_channels)
    return LD.LSSViewTransformerBEVDepth_racformer(grid_config=grid, input_size=(H, W), downsample=int(fx["downsample"]),
                                                   in_channels=in_channels, out_channels=out_channels, depth_net=net,
                                                   loss_depth_weight=float(fx["loss_depth_weight"]), **kw)


@pytest.mark.parametrize("tag", TAGS)
def test_pooling_and_index_maps_equal_the_reference(fixtures, tag):
    fx = fixtures[tag]
    grid, ds = R.golden_grid(fx), int(fx["downsample"])
    n_rcs = int(grid["rcs"][2])
    for src, inds, pooled in (("radar_depth", "rad_inds", "radar_pooled"), ("lidar_depth", "label_inds", "label_pooled")):
        p = R.pooled_depth(maps(fx, src), ds)
        assert np.array_equal(p.numpy(), fx[pooled]) and np.array_equal(R.depth_bins(p, grid["depth"]).numpy(), fx[inds])
    cls = R.rcs_class(maps(fx, "radar_rcs"), ds, grid["rcs"])
    assert int(cls.min()) >= 0 and np.array_equal(R.rcs_one_hot(cls, n_rcs).numpy(), fx["rcs_one_hot"])
    # the package's CPU route: functional layer and module
    pooled, bins, cls2 = LD.pool_bins(maps(fx, "radar_depth"), maps(fx, "radar_rcs"), grid, ds)
    assert bins.dtype == cls2.dtype == torch.int32
    assert np.array_equal(pooled.numpy(), fx["radar_pooled"]) and np.array_equal(bins.numpy(), fx["rad_inds"])
    assert torch.equal(cls2.long(), cls)
    m = module_for(fx)
    inds, pooled = m.get_downsampled_depth(torch.from_numpy(fx["lidar_depth"]), 0)
    assert inds.dtype == torch.int64 and np.array_equal(inds.numpy(), fx["label_inds"])
    assert np.array_equal(pooled.numpy(), fx["label_pooled"])
    one_hot = m.get_downsampled_rcs(torch.from_numpy(fx["radar_rcs"]), ds)
    assert one_hot.dtype == torch.float32 and np.array_equal(one_hot.numpy(), fx["rcs_one_hot"])


@pytest.mark.parametrize("tag", TAGS)
def test_prior_tensors_equal_the_reference(fixtures, tag):
    fx = fixtures[tag]
    D = int(fx["grid_depth"][2])
    bins = torch.from_numpy(fx["rad_inds"])
    cls = R.rcs_class(maps(fx, "radar_rcs"), int(fx["downsample"]), R.golden_grid(fx)["rcs"])
    gout = torch.from_numpy(fx["prior_gout"])
    pixels = bins.numel()
    tol = pixels * U * float(gout.abs().sum(dim=(0, 2, 3)).max())
    routes = {"restatement": lambda w, b: torch.cat(R.prior(bins, cls, w.view(w.shape[0], -1), b, D), 1),
              "package": lambda w, b: LD.radar_prior(bins.int(), cls.int(), w, b, D)}
    for name, route in routes.items():
        w = torch.from_numpy(fx["rcs_weight"]).clone().requires_grad_(True)
        b = torch.from_numpy(fx["rcs_bias"]).clone().requires_grad_(True)
        out = route(w, b)
        assert np.array_equal(out[:, :D + 1].detach().numpy(), fx["rad_dep_grids"]), name
        assert np.array_equal(out[:, D + 1:].detach().numpy(), fx["rcs_embedding"]), name          # a gather plus one add
        gw, gb = torch.autograd.grad((out[:, D + 1:] * gout).sum(), (w, b))
        err_w = float((gw - torch.from_numpy(fx["grad_rcs_weight"])).abs().max())
        err_b = float((gb - torch.from_numpy(fx["grad_rcs_bias"])).abs().max())
        print(f"{tag} {name}: grad_weight {err_w:.3g}, grad_bias {err_b:.3g} (allowed {tol:.3g})")
        assert gw.shape == w.shape and err_w <= tol and err_b <= tol


@pytest.mark.parametrize("tag", TAGS)
def test_depth_loss_and_gradient_match_the_reference(fixtures, tag):
    fx = fixtures[tag]
    labels = torch.from_numpy(fx["label_inds"])
    D = int(fx["grid_depth"][2])
    weight = float(fx["loss_depth_weight"])
    n = D + labels.numel()
    want, want_grad = float(fx["loss"]), torch.from_numpy(fx["grad_preds"])
    m = module_for(fx)
    routes = {"restatement": lambda p: R.depth_loss(p, labels, weight)[0],
              "package": lambda p: LD.depth_loss(p, labels.int(), 0.25, 2.0, weight),
              "module": lambda p: m.get_depth_loss(torch.from_numpy(fx["lidar_depth"]), p)}
    for name, route in routes.items():
        preds = torch.from_numpy(fx["depth_preds"]).clone().requires_grad_(True)
        loss = route(preds)
        (grad,) = torch.autograd.grad(loss, preds)
        err, gerr = abs(float(loss.detach()) - want), float((grad - want_grad).abs().max())
        tol, gtol = n * U * abs(want), n * U * float(want_grad.abs().max())
        print(f"{tag} {name}: loss {err:.3g} (allowed {tol:.3g}), gradient {gerr:.3g} (allowed {gtol:.3g})")
        assert loss.dim() == 0 and err <= tol and gerr <= gtol
        bg = (labels >= D).unsqueeze(1).expand_as(grad)
        assert int(bg.sum()) > 0 or tag == "a"
        assert (grad[bg] == 0).all()
    # float64 restatement: the float32 one is its rounding
    l64, _ = R.depth_loss(torch.from_numpy(fx["depth_preds"]), labels, weight, dtype=torch.float64)
    assert abs(float(l64) - want) <= n * U * abs(want)


def test_depth_bin_edges_equal_the_numpy_yardstick(fixtures):
    """Every constructed bin edge d_k, k = 0..97, with its two float32 neighbours, and 0, 0.5, 1e5, inf, nan, a negative value:
    the routes equal the IEEE float32 sequence in numpy exactly and stay within one bin of the reference's own run (whose
    float32 sqrt on the CPU is not correctly rounded)."""
    grid = dict(depth=[1.0, 65.0, 96.0])
    d = R.edge_depths(grid["depth"])
    assert np.array_equal(d, fixtures["edges"]["depths"], equal_nan=True) and d.size == 3 * 98 + 6
    want = R.depth_bins_numpy(d, grid["depth"])
    t = torch.from_numpy(d)
    routes = {"restatement": R.depth_bins(t.clone(), grid["depth"]).numpy(),
              "package": LD.pool_bins(t.view(1, 1, -1), None, grid, 1)[1].view(-1).long().numpy()}
    ref = fixtures["edges"]["inds"]
    moved = int((ref != want).sum())
    print(f"{d.size} edge depths: the reference's run differs from numpy at {moved}")
    for name, got in routes.items():
        assert np.array_equal(got, want), name
        assert np.abs(got - ref).max() <= 1, name
    assert np.abs(want[:97] - np.arange(97)).max() <= 1 and want[97] == 96              # d_k: the edge below bin k; d_97 is past the range
    assert want[-6:].tolist() == [96, 96, 96, 96, 96, 96]                               # 0, 0.5, 1e5, inf, nan, -3: no bin


def test_blocks_without_a_class_get_minus_one():
    """Where the reference's F.one_hot raises -- all values below the range, a maximum >= the upper bound, NaN -- the class is -1:
    an all-zero one-hot row and the bias alone in the embedding."""
    grid = dict(depth=[1.0, 65.0, 24.0], rcs=[-64, 64, 64])
    rcs = torch.full((1, 4, 8), -100.0)
    rcs[0, 0, 2] = 64.0                 # block 1: maximum == hi
    rcs[0, 1, 5] = float("nan")         # block 2
    rcs[0, 3, 7] = 63.999               # block 3: the last class
    rcs[0, 2, 6] = -64.0                # (the same block: the maximum wins)
    depth = torch.zeros(1, 4, 8)
    depth[0, 2, 1], depth[0, 1, 0] = 30.0, 12.0
    depth[0, 0, 4] = float("nan")
    pooled, bins, cls = LD.pool_bins(depth, rcs, grid, 2)
    want = R.rcs_class(rcs, 2, grid["rcs"])
    assert cls.view(-1).tolist() == [-1, -1, -1, -1, -1, -1, -1, 63] and torch.equal(cls.long(), want)
    assert pooled[0, 0, 0] == 12.0 and pooled[0, 1, 0] == 30.0 and pooled[0, 0, 1] == 1e5 and torch.isnan(pooled[0, 0, 2])
    assert bins[0, 0, 1] == 24 and bins[0, 0, 2] == 24 and 0 <= bins[0, 0, 0] < bins[0, 1, 0] < 24
    w, b = torch.randn(32, 64, 1, 1), torch.randn(32)
    prior = LD.radar_prior(bins, cls, w, b, 24)
    assert prior.shape == (1, 25 + 32, 2, 4)
    assert torch.equal(prior[0, 25:, 0, 0], b) and torch.equal(prior[0, 25:, 1, 3], w[:, 63, 0, 0] + b)
    assert torch.equal(prior[0, :25].sum(0), torch.ones(2, 4))
    with pytest.raises(ValueError, match="multiple of downsample"):
        LD.pool_bins(depth, rcs, grid, 3)


def test_module_on_cpu_tensors(fixtures):
    fx = fixtures["a"]
    m = module_for(fx)
    keys = sorted(k for k in m.state_dict() if not k.startswith("depth_net."))
    assert keys == [str(k) for k in fx["state_keys"]] == ["frustum", "rcs_embedding.bias", "rcs_embedding.weight"]
    assert any(k.startswith("depth_net.") for k in m.state_dict())
    assert m.rcs_embedding.weight.shape == (32, 64, 1, 1)
    B, N, H, W = fx["radar_depth"].shape
    ds, D = int(fx["downsample"]), int(fx["grid_depth"][2])
    metas = syn.make_lss_view_inputs(n_cams=N, batch=B, input_hw=(H, W), downsample=ds, channels=8,
                                     grid_config=dict(GRID_XYZ, depth=[1.0, 65.0, float(D)]))["img_metas"]
    mlp_input = m.get_mlp_input(metas)
    assert mlp_input.shape == (B, N, 9) and mlp_input.dtype == torch.float32
    x = torch.from_numpy(syn.rng_normal(5, (B, N, 16, H // ds, W // ds))).requires_grad_(True)
    bev, depth_digit = m(x, torch.from_numpy(fx["radar_depth"]), torch.from_numpy(fx["radar_rcs"]), metas, mlp_input)
    assert bev.shape == (B, 8 * m.grid.size[2], m.grid.size[1], m.grid.size[0]) and depth_digit.shape == (B * N, D, H // ds, W // ds)
    loss = m.get_depth_loss(torch.from_numpy(fx["lidar_depth"]), depth_digit)
    (bev.square().sum() + loss).backward()
    assert bev.abs().sum() > 0 and x.grad.abs().sum() > 0
    assert m.rcs_embedding.weight.grad.abs().sum() > 0 and m.rcs_embedding.bias.grad.abs().sum() > 0
    with pytest.raises(TypeError, match="depth_net"):
        LD.LSSViewTransformerBEVDepth_racformer(grid_config=dict(GRID_XYZ, **R.golden_grid(fx)), input_size=(H, W), downsample=ds)


def test_argument_errors_need_no_gpu():
    """Null pointers, maps that are no multiple of ds and D < 1 are refused before any HIP call."""
    from racformer_amd import _lib
    lib = _lib.lib()
    p = ctypes.c_void_p(16)
    args = (1.0, 0.0137, 96, -64.0, -66.0, 2.0, 64, None)
    assert lib.rac_lss_pool_bins_fwd(None, None, None, None, None, 1, 16, 16, 4, *args) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_lss_pool_bins_fwd(p, None, None, p, None, 1, 16, 16, 4, *args) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_lss_pool_bins_fwd(p, p, p, p, p, 1, 16, 18, 4, *args) == -1 and b"not a multiple of ds" in lib.rac_last_error()
    assert lib.rac_lss_pool_bins_fwd(p, p, p, p, p, 1, 16, 16, 0, *args) == -1
    assert lib.rac_lss_pool_bins_fwd(p, p, p, p, p, 1, 4096, 4096, 2048, *args) != 0 and b"exceeds" in lib.rac_last_error()
    assert lib.rac_lss_prior_fwd(p, p, p, None, p, 1, 12, 24, 32, 64, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_lss_prior_fwd(p, p, p, p, p, 1, 12, 0, 32, 64, None) == -1 and b"D=0" in lib.rac_last_error()
    assert lib.rac_lss_prior_bwd(p, None, p, p, p, 1, 12, 24, 32, 64, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_lss_prior_bwd(p, p, p, p, p, 1, 12, 24, 32, 257, None) != 0 and b"exceeds" in lib.rac_last_error()
    assert lib.rac_lss_depth_loss_fwd(p, None, p, p, None, p, p, 1, 24, 12, 0.25, 2.0, 3.0, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_lss_depth_loss_fwd(p, p, p, p, None, p, p, 1, 0, 12, 0.25, 2.0, 3.0, None) == -1 and b"D=0" in lib.rac_last_error()
    assert lib.rac_lss_depth_loss_fwd(p, p, p, p, None, p, p, 1, 24, 12, 0.25, 1.5, 3.0, None) != 0 and b"gamma" in lib.rac_last_error()
    assert lib.rac_lss_depth_loss_bwd(p, p, None, p, 8, None) == -1 and b"null pointer" in lib.rac_last_error()
