"""The CPU restatement of the Lift-Splat view transform (tests/lss_view_ref.py) against the reference's own run
(tests/golden/lss_view_small.npz, written by tests/golden/gen_golden_lss_view.py), and the module's constructor state."""
import pytest
import torch

import lss_view_ref as R
from racformer_amd.lss_view import LSSViewTransformer_racformer

TAGS = ("a", "b")


@pytest.fixture(scope="module")
def fixtures(golden_dir):
    out = {}
    for tag in TAGS:
        fx = R.golden_fixture(golden_dir, tag)
        fx["axes"] = R.frustum_axes(fx["frustum"])
        fx["grid"] = R.grid_of(fx["grid_config"])
        fx["m"] = R.img2lidar_f32(fx["img_metas"])
        fx["batch"] = len(fx["img_metas"])
        out[tag] = fx
    return out


def golden_cells(fx):
    cells = torch.full((fx["coor"].numel() // 3,), -1, dtype=torch.int64)
    cells[fx["ranks_depth"].long()] = fx["ranks_bev"].long()
    return cells


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_the_reference(fixtures, tag):
    fx = fixtures[tag]
    lower, interval, size = fx["grid"]
    B = fx["batch"]
    BN, D, H, W = fx["depth_digit"].shape
    # coordinates: 1e-5 relative to the point's largest component (a component near zero has no relative scale of its own)
    xyz = R.lidar_points(fx["m"], *fx["axes"])
    ref = fx["coor"].reshape(xyz.shape)
    scale = ref.abs().amax(-1, keepdim=True).clamp(min=1.0)
    rel = ((xyz - ref).abs() / scale).max().item()
    print(f"{tag}: coordinates, largest relative deviation {rel:.3g}")
    assert rel <= 1e-5
    # kept set and every point's cell, exactly
    scaled = R.scaled_coords(fx["m"], *fx["axes"], lower, interval)
    cells = R.cells_of(scaled, size, BN // B)
    assert torch.equal(cells, golden_cells(fx))
    # per cell the SET of ranks_depth (the reference's argsort is not stable: order inside a cell is unspecified there)
    rb, rd, rf, starts, lengths = R.tables_of(cells, D, H * W)
    g_rb, g_rd, g_rf = fx["ranks_bev"].long(), fx["ranks_depth"].long(), fx["ranks_feat"].long()
    order = torch.argsort(g_rb * cells.numel() + g_rd)
    assert torch.equal(g_rb[order], rb) and torch.equal(g_rd[order], rd) and torch.equal(g_rf[order], rf)
    assert torch.equal(g_rb, rb)                                         # sorted by cell there too
    # interval tables, consistent with the sets
    assert torch.equal(fx["interval_starts"].long(), starts) and torch.equal(fx["interval_lengths"].long(), lengths)
    assert int(lengths.sum()) == rd.numel() and torch.equal(rb[starts], torch.unique(rb))
    # output: the reference's float32 run may be 4 x E_ref from the float64 restatement, E_ref = the float32 restatement's own
    # error (both are sequential float32 sums; they differ in the order inside a cell)
    out64 = R.splat(fx["depth_digit"], fx["tran_feat"], cells, B, size, torch.float64)
    out32 = R.splat(fx["depth_digit"], fx["tran_feat"], cells, B, size, torch.float32)
    e_ref = (out32.double() - out64).abs().max().item()
    err = (fx["out"].double() - out64).abs().max().item()
    print(f"{tag}: output, E_ref {e_ref:.3g}, reference's float32 run {err:.3g}")
    assert fx["out"].shape == out64.shape and e_ref > 0 and err <= 4 * e_ref
    assert (fx["out"][out64 == 0] == 0).all()                            # empty cells


def test_truncation_quirk_is_present(fixtures):
    """A scaled coordinate in (-1, 0) truncates to cell 0 and the point is kept: pinned, not fixed."""
    for tag in TAGS:
        fx = fixtures[tag]
        lower, interval, size = fx["grid"]
        scaled = R.scaled_coords(fx["m"], *fx["axes"], lower, interval)
        cells = R.cells_of(scaled, size, fx["depth_digit"].shape[0] // fx["batch"])
        n = int(R.quirk_points(scaled, cells).sum())
        assert n == int(fx["n_quirk"])
        if tag == "a":
            assert n > 0
            floored = torch.floor(scaled)              # a floor would have dropped them
            assert int(((floored < 0).any(-1).reshape(-1) & (cells >= 0)).sum()) == n


@pytest.mark.parametrize("tag", TAGS)
def test_module_state_matches_the_reference(fixtures, tag):
    fx = fixtures[tag]
    m = LSSViewTransformer_racformer(fx["grid_config"], fx["input_size"], downsample=fx["downsample"], in_channels=16,
                                     out_channels=fx["tran_feat"].shape[1])
    assert sorted(m.state_dict().keys()) == fx["state_keys"] == ["depth_net.bias", "depth_net.weight", "frustum"]
    assert m.frustum.dtype == torch.float32 and torch.equal(m.frustum.data, fx["frustum"])        # bit for bit
    assert not m.frustum.requires_grad
    assert m.grid == R.grid_of(fx["grid_config"])
    for mine, ref in zip((m.depth_table, m.v_table, m.u_table), fx["axes"]):
        assert torch.equal(mine, ref)


def test_cpu_tensors_are_refused(fixtures):
    fx = fixtures["b"]
    m = LSSViewTransformer_racformer(fx["grid_config"], fx["input_size"], downsample=fx["downsample"], in_channels=16,
                                     out_channels=4)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        m.view_transform(None, fx["depth_digit"], fx["tran_feat"], fx["img_metas"])
