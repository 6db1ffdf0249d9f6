"""The Lift-Splat view transform on the GPU (racformer_amd/lss_view.py, csrc/lss_view.hip) against the CPU restatement
(tests/lss_view_ref.py, pinned to the reference by tests/test_lss_view_ref.py).

Tolerances are measured per rig, not fixed: E_ref is the largest absolute error of the float32 CPU restatement (sequential
sums, like the reference's kernel) against the float64 restatement on the same cells; the kernel may reach 4 x E_ref, the
project's ratio for a reordered fp32 sum (tests/test_fused_gpu.py) -- chunked and sequential sums differ by rounding order only.
With RAC_LSS_VIEW_ERRORS=<file> set, every (E_ref, kernel error) pair of a session is written to that file as JSON
(tools/lss_view_bench.py --errors copies it into the record; committed copy: profiles/lss_view_f8.json)."""
import json
import os

import pytest
import torch

import lss_view_ref as R
from racformer_amd import lss_view as LV
from racformer_amd import synthetic as syn
from racformer_amd.bev_pool import bev_pool_v2

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAND, BAND_CAP = 1e-3, 0.02
RATIO = 4.0
F8_WORST_CELL = 4416

CROWDED = dict(x=[-51.2, 51.2, 51.2], y=[-51.2, 51.2, 51.2], z=[-5.0, 3.0, 8.0], depth=[1.0, 65.0, 96.0])
SPARSE = dict(x=[-6.4, 6.4, 0.1], y=[-6.4, 6.4, 0.1], z=[-5.0, 1.0, 6.0], depth=[1.0, 65.0, 24.0])
SYNTHETIC = {
    "f8": dict(channels=64),                                                  # 6 cameras, D=96, 16x44, 128x128 cells: 405 504 points
    "crowded": dict(n_cams=2, input_hw=(128, 192), grid_config=CROWDED, yaws=(0.5,), seed=5),     # 2x2 cells of 51.2 m
    "sparse": dict(n_cams=1, batch=2, input_hw=(32, 48), grid_config=SPARSE, yaws=(0.07, 0.3), seed=6),   # N=1, lone points
}
RIGS = ("a", "b", "f8", "crowded", "sparse")
ERRORS = {}


class Rig:
    """Inputs, the kernel's tables and the float64 view of one rig; CPU references are computed once and shared."""

    def __init__(self, name, golden_dir):
        self.name = name
        if name in SYNTHETIC:
            inp = syn.make_lss_view_inputs(**SYNTHETIC[name])
        else:
            inp = R.golden_fixture(golden_dir, name)
        self.inp = inp
        self.module = LV.LSSViewTransformer_racformer(inp["grid_config"], inp["input_size"], downsample=inp["downsample"],
                                                      in_channels=16, out_channels=inp["tran_feat"].shape[1])
        self.axes = R.frustum_axes(self.module.frustum.data)
        self.lower, self.interval, self.size = R.grid_of(inp["grid_config"])
        self.grid = self.module.grid
        self.batch = len(inp["img_metas"])
        self.m = R.img2lidar_f32(inp["img_metas"])
        self.logits = inp["depth_digit"]
        self.shape = tuple(self.logits.shape)
        self.n_cams = self.shape[0] // self.batch
        self.tables_dev = LV.FrustumTables(*(t.to(DEV) for t in self.axes))
        self.m_dev = self.m.to(DEV)
        self.ranks = LV.lss_rank_tables(self.m_dev, self.tables_dev, self.grid, self.batch, self.shape)
        torch.cuda.synchronize()
        self.cells = self.ranks.cells.cpu().long()
        self._feat, self._fwd, self._bwd = {}, {}, {}

    def feat(self, c):
        """[B*N, c, H, W] features: the rig's own where the width matches, seeded N(0,1) otherwise"""
        if c not in self._feat:
            own = self.inp["tran_feat"]
            bn, _, h, w = self.shape
            self._feat[c] = own if own.shape[1] == c else torch.from_numpy(syn.rng_normal(900 + c, (bn, c, h, w)))
        return self._feat[c]

    def forward_ref(self, c):
        """(out64, E_ref) on the KERNEL's cells, so that band points do not enter"""
        if c not in self._fwd:
            o64 = R.splat(self.logits, self.feat(c), self.cells, self.batch, self.size, torch.float64)
            o32 = R.splat(self.logits, self.feat(c), self.cells, self.batch, self.size, torch.float32)
            self._fwd[c] = (o64, (o32.double() - o64).abs().max().item())
        return self._fwd[c]

    def gout(self, c):
        X, Y, Z = self.size
        return torch.from_numpy(syn.rng_normal(700 + c, (self.batch, Z * c, Y, X)))

    def backward_ref(self, c):
        """float64 autograd of the restatement, and the float32 restatement's own error against it, per gradient"""
        if c not in self._bwd:
            res = {}
            for dt in (torch.float64, torch.float32):
                lg = self.logits.to(dt).requires_grad_(True)
                ft = self.feat(c).to(dt).requires_grad_(True)
                out = R.splat(lg, ft, self.cells, self.batch, self.size, dt)
                res[dt] = torch.autograd.grad((out * self.gout(c).to(dt)).sum(), (lg, ft))
            g64, g32 = res[torch.float64], res[torch.float32]
            self._bwd[c] = (g64, tuple((a.double() - b).abs().max().item() for a, b in zip(g32, g64)))
        return self._bwd[c]

    def run(self, c, backward=False):
        lg = self.logits.to(DEV).requires_grad_(backward)
        ft = self.feat(c).to(DEV).requires_grad_(backward)
        out = LV.lss_view_transform(lg, ft, self.m_dev, self.tables_dev, self.grid, self.batch, ranks=self.ranks)
        if not backward:
            return out
        gl, gf = torch.autograd.grad(out, (lg, ft), self.gout(c).to(DEV))
        return out, gl, gf


_RIGS = {}


@pytest.fixture(scope="module")
def rigs(golden_dir):
    def get(name):
        if name not in _RIGS:
            _RIGS[name] = Rig(name, golden_dir)
        return _RIGS[name]
    yield get
    _RIGS.clear()
    path = os.environ.get("RAC_LSS_VIEW_ERRORS")
    if ERRORS and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(ratio_allowed=RATIO, errors=ERRORS), f, indent=1, sort_keys=True)


def record(key, e_ref, err):
    ERRORS[key] = dict(E_ref=e_ref, kernel=err)
    print(f"{key}: E_ref {e_ref:.3g}, kernel {err:.3g} (allowed {RATIO * e_ref:.3g})")


# ------------------------------------------------------------------------------------------------------------ 1. cells
@pytest.mark.parametrize("name", RIGS)
def test_1_cells(rigs, name):
    rig = rigs(name)
    scaled = R.scaled_coords(rig.m, *rig.axes, rig.lower, rig.interval, torch.float64)
    want = R.cells_of(scaled, rig.size, rig.n_cams)
    band = ((scaled - scaled.round()).abs() <= BAND).any(-1).reshape(-1)
    share = band.float().mean().item()
    print(f"{name}: {band.numel()} points, {int((want >= 0).sum())} kept, band share {100 * share:.2f} %, "
          f"{int((rig.cells != want).sum())} cells differ from float64")
    assert share <= BAND_CAP, "a condition on the rig, not a tolerance: change the rig's yaw"
    assert torch.equal(rig.cells[~band], want[~band])                    # dropped points included
    # inside the band: one of the adjacent candidates (the cell of the coordinate moved by the band's width on any axes)
    idx = torch.nonzero(band & (rig.cells != want)).flatten()
    if idx.numel():
        pts = scaled.reshape(-1, 3)[idx]
        bn = idx // (scaled.numel() // 3 // scaled.shape[0])
        ok = torch.zeros(idx.numel(), dtype=torch.bool)
        X, Y, Z = rig.size
        for dx in (-BAND, 0.0, BAND):
            for dy in (-BAND, 0.0, BAND):
                for dz in (-BAND, 0.0, BAND):
                    q = (pts + torch.tensor([dx, dy, dz], dtype=torch.float64)).long()
                    kept = ((q >= 0) & (q < torch.tensor([X, Y, Z]))).all(-1)
                    cell = (((bn // rig.n_cams) * Z + q[:, 2]) * Y + q[:, 1]) * X + q[:, 0]
                    ok |= torch.where(kept, cell, torch.full_like(cell, -1)) == rig.cells[idx]
        assert ok.all()
    if name == "crowded":
        assert int(torch.bincount(rig.cells[rig.cells >= 0]).max()) >= F8_WORST_CELL
    if name == "sparse":
        cnt = torch.bincount(rig.cells[rig.cells >= 0], minlength=rig.batch * rig.size[0] * rig.size[1] * rig.size[2])
        assert int((cnt == 1).sum()) > 0 and (cnt == 0).float().mean() > 0.5


# ------------------------------------------------------------------------------------------------------------ 2. tables
@pytest.mark.parametrize("name", RIGS)
def test_2_tables(rigs, name):
    rig = rigs(name)
    bn, D, H, W = rig.shape
    rb, rd, rf, starts, lengths, counts = (t.cpu().long() for t in rig.ranks[1:])
    n_kept, n_occ = int(counts[0]), int(counts[1])
    n_points, n_cells = rig.cells.numel(), rig.batch * rig.size[0] * rig.size[1] * rig.size[2]
    assert rb.numel() == rd.numel() == rf.numel() == n_points and starts.numel() == lengths.numel() == min(n_points, n_cells)
    # the counts and tables are the restatement's on the kernel's cells (test 1 reconciles those with float64)
    w_rb, w_rd, w_rf, w_starts, w_lengths = R.tables_of(rig.cells, D, H * W)
    assert n_kept == w_rd.numel() == int((rig.cells >= 0).sum()) and n_occ == w_starts.numel()
    k_rb, k_rd, k_rf, k_starts, k_lengths = rb[:n_kept], rd[:n_kept], rf[:n_kept], starts[:n_occ], lengths[:n_occ]
    assert (k_rb[1:] >= k_rb[:-1]).all()                                                   # sorted by cell
    same = k_rb[1:] == k_rb[:-1]
    assert (k_rd[1:][same] > k_rd[:-1][same]).all()                                        # ascending inside a cell
    assert int(k_starts[0]) == 0 if n_occ else True
    assert torch.equal(k_starts[1:], (k_starts + k_lengths)[:-1]) and int(k_lengths.sum()) == n_kept    # tile [0, n_kept)
    assert (k_lengths > 0).all() and torch.equal(k_rb[k_starts], torch.unique(k_rb))
    assert torch.equal(k_rf, (k_rd // (D * H * W)) * (H * W) + k_rd % (H * W))
    assert torch.equal(rig.cells[k_rd], k_rb)
    for got, want in ((k_rb, w_rb), (k_rd, w_rd), (k_rf, w_rf), (k_starts, w_starts), (k_lengths, w_lengths)):
        assert torch.equal(got, want)
    # the documented padding
    assert (rb[n_kept:] == -1).all() and (rd[n_kept:] == -1).all() and (rf[n_kept:] == -1).all()
    assert (starts[n_occ:] == 0).all() and (lengths[n_occ:] == 0).all()
    # the trimmed tables drive the existing operator to the same map
    c = rig.inp["tran_feat"].shape[1]
    t = LV.lss_rank_tables(rig.m_dev, rig.tables_dev, rig.grid, rig.batch, rig.shape, trim=True)
    assert t.ranks_bev.numel() == n_kept and t.interval_starts.numel() == n_occ
    X, Y, Z = rig.size
    depth = rig.logits.to(DEV).softmax(dim=1).view(rig.batch, rig.n_cams, D, H, W)
    feat = rig.feat(c).to(DEV).view(rig.batch, rig.n_cams, c, H, W).permute(0, 1, 3, 4, 2).contiguous()
    pooled = bev_pool_v2(depth, feat, t.ranks_depth, t.ranks_feat, t.ranks_bev, (rig.batch, Z, Y, X, c), t.interval_starts,
                         t.interval_lengths)                                                # [B, C, Z, Y, X]
    pooled = torch.cat(pooled.unbind(dim=2), 1).cpu()
    fused = rig.run(c).cpu()
    _, e_ref = rig.forward_ref(c)
    diff = (pooled - fused).abs().max().item()
    print(f"{name}: bev_pool_v2 on the tables against the fused path: {diff:.3g} (allowed {RATIO * e_ref:.3g})")
    assert diff <= RATIO * e_ref


# ------------------------------------------------------------------------------------------------------------ 3. forward
FORWARD = [("a", 8), ("b", 4), ("f8", 64), ("crowded", 256), ("crowded", 80), ("crowded", 64), ("sparse", 256), ("sparse", 80),
           ("a", 80), ("b", 320)]


@pytest.mark.parametrize("name,c", FORWARD)
def test_3_forward(rigs, name, c):
    rig = rigs(name)
    out64, e_ref = rig.forward_ref(c)
    out = rig.run(c).cpu()
    err = (out.double() - out64).abs().max().item()
    record(f"forward:{name}:C{c}", e_ref, err)
    assert out.shape == out64.shape
    X, Y, Z = rig.size
    cnt = torch.bincount(rig.cells[rig.cells >= 0], minlength=rig.batch * X * Y * Z).view(rig.batch, Z, 1, Y, X)
    empty = (cnt == 0).expand(rig.batch, Z, c, Y, X).reshape(out.shape)
    assert (out[empty] == 0).all() and (int(empty.sum()) > 0 or name == "crowded")              # empty cells exactly zero
    assert err <= RATIO * e_ref
    if name in ("a", "b") and c == rig.inp["tran_feat"].shape[1]:
        gold = (rig.inp["out"].double() - out64).abs().max().item()                              # the reference's own run
        assert gold <= RATIO * e_ref


@pytest.mark.parametrize("c", [0, 2, 6, 81, 324, 512])
def test_3_refused_widths_launch_nothing(rigs, c):
    from racformer_amd import _lib
    rig = rigs("b")
    out = torch.full((64,), 7.0, device=DEV)
    one = torch.zeros(64, device=DEV)
    idx = torch.zeros(64, dtype=torch.int32, device=DEV)
    p = _lib.ptr
    rc = _lib.lib().rac_lss_splat_fwd(p(one), p(one), p(one), p(idx), p(idx), p(idx), p(idx), p(idx), p(idx), p(idx), p(one), p(out),
                                      1, 1, c, 1, 1, 1, _lib.stream_ptr())
    assert rc != 0 and b"C=" in _lib.lib().rac_last_error()
    rc = _lib.lib().rac_lss_view_bwd(p(one), p(one), p(one), p(one), p(idx), p(out), p(out), 1, c, 1, 1, _lib.stream_ptr())
    assert rc != 0
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    if c:
        with pytest.raises(RuntimeError, match="rac_lss_splat_fwd"):
            bn, _, h, w = rig.shape
            LV.lss_view_transform(rig.logits.to(DEV), torch.zeros(bn, c, h, w, device=DEV), rig.m_dev, rig.tables_dev, rig.grid,
                                  rig.batch, ranks=rig.ranks)


# ------------------------------------------------------------------------------------------------------------ 4. backward
BACKWARD = [("a", 8), ("b", 4), ("f8", 64), ("crowded", 256), ("crowded", 80), ("sparse", 64), ("sparse", 320)]


@pytest.mark.parametrize("name,c", BACKWARD)
def test_4_backward(rigs, name, c):
    rig = rigs(name)
    (gl64, gf64), (e_gl, e_gf) = rig.backward_ref(c)
    _, gl, gf = rig.run(c, backward=True)
    gl, gf = gl.cpu(), gf.cpu()
    err_gl, err_gf = (gl.double() - gl64).abs().max().item(), (gf.double() - gf64).abs().max().item()
    record(f"grad_logits:{name}:C{c}", e_gl, err_gl)
    record(f"grad_feat:{name}:C{c}", e_gf, err_gf)
    assert err_gl <= RATIO * e_gl and err_gf <= RATIO * e_gf
    bn, D, H, W = rig.shape
    kept = (rig.cells >= 0).view(bn, D, H, W)
    any_kept = kept.any(1, keepdim=True)
    # a dropped bin of a pixel that has kept bins gets its gradient through the softmax: non-zero, equal to the reference's
    dropped_live = (~kept) & any_kept
    assert int(dropped_live.sum()) > 0
    assert (gl64[dropped_live] != 0).all() and (gl[dropped_live] != 0).all()
    assert (gl.double() - gl64)[dropped_live].abs().max().item() <= RATIO * e_gl
    # a pixel without a kept bin: zero gradients
    dead = ~any_kept
    assert (gl[dead.expand_as(gl)] == 0).all() and (gf[dead.expand(bn, c, H, W)] == 0).all()
    if name == "sparse":
        assert int(dead.sum()) > 0


# ------------------------------------------------------------------------------------------------------------ 5. determinism
def test_5_two_runs_give_the_same_bits(rigs):
    rig = rigs("crowded")
    first = [t.clone() for t in rig.run(256, backward=True)]
    ranks2 = LV.lss_rank_tables(rig.m_dev, rig.tables_dev, rig.grid, rig.batch, rig.shape)
    for a, b in zip(rig.ranks, ranks2):
        assert torch.equal(a, b)                                         # the unordered fill leaves no trace in the tables
    second = rig.run(256, backward=True)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 6. graph capture
def test_6_graph_capture_and_replay_on_other_inputs(rigs):
    """Tables, forward and backward captured on one stream; replayed after the logits, the features and the device matrices were
    overwritten in place with another sample's: equal to an eager autograd run on those, bit for bit -- no launch is sized by a
    count read back (the two samples keep different numbers of points).  The captured region calls the operator's forward and
    backward launches directly (lss_view_forward / lss_view_backward, what the autograd Function calls), on the capturing thread."""
    rig = rigs("a")
    c = 8
    other = syn.make_lss_view_inputs(n_cams=2, batch=2, input_hw=(64, 96), channels=c, yaws=(0.9, -0.4), seed=21,
                                     grid_config=rig.inp["grid_config"])
    m2 = R.img2lidar_f32(other["img_metas"]).to(DEV)
    gout = rig.gout(c).to(DEV)

    def eager(logits, feat, m):
        lg, ft = logits.to(DEV).requires_grad_(True), feat.to(DEV).requires_grad_(True)
        ranks = LV.lss_rank_tables(m, rig.tables_dev, rig.grid, rig.batch, rig.shape)
        out = LV.lss_view_transform(lg, ft, m, rig.tables_dev, rig.grid, rig.batch, ranks=ranks)
        return (out,) + torch.autograd.grad(out, (lg, ft), gout) + (ranks.counts,)

    want1 = [t.clone() for t in eager(rig.logits, rig.feat(c), rig.m_dev)]
    want2 = [t.clone() for t in eager(other["depth_digit"], other["tran_feat"], m2)]
    assert not torch.equal(want1[3], want2[3])                           # another number of kept points
    s_lg, s_ft, s_m = rig.logits.to(DEV), rig.feat(c).to(DEV), rig.m_dev.clone()

    def step():
        ranks = LV.lss_rank_tables(s_m, rig.tables_dev, rig.grid, rig.batch, rig.shape)
        out, stats, feat_cl = LV.lss_view_forward(s_lg, s_ft, ranks, rig.grid, rig.batch)
        return (out,) + LV.lss_view_backward(gout, s_lg, stats, feat_cl, ranks.cells, rig.grid, rig.batch) + (ranks.counts,)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        got = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(got, want1):
        assert torch.equal(a, b)
    s_lg.copy_(other["depth_digit"])
    s_ft.copy_(other["tran_feat"])
    s_m.copy_(m2)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(got, want2):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 7. module
def test_7_module_accelerate_and_cpu_tensors(rigs):
    rig = rigs("a")
    inp = rig.inp
    c = inp["tran_feat"].shape[1]
    bn, D, H, W = rig.shape
    x = torch.from_numpy(syn.rng_normal(31, (rig.batch, rig.n_cams, 16, H, W)))
    other = syn.make_lss_view_inputs(n_cams=2, batch=2, input_hw=(64, 96), channels=c, yaws=(0.9, -0.4),
                                     grid_config=inp["grid_config"])["img_metas"]
    mods = {}
    torch.manual_seed(5)
    for acc in (False, True):
        m = LV.LSSViewTransformer_racformer(inp["grid_config"], inp["input_size"], downsample=inp["downsample"], in_channels=16,
                                            out_channels=c, accelerate=acc)
        if mods:
            m.load_state_dict(mods[False].state_dict())                  # the same depth_net weights in both
        mods[acc] = m.to(DEV)
    outs = {acc: m(x.to(DEV), inp["img_metas"]) for acc, m in mods.items()}
    assert outs[False][0].shape == (rig.batch, c * rig.size[2], rig.size[1], rig.size[0])
    assert outs[False][1].shape == (bn, D, H, W)
    assert torch.equal(outs[False][0], outs[True][0]) and torch.equal(outs[False][1], outs[True][1])
    assert outs[False][0].abs().sum() > 0
    again = {acc: m(x.to(DEV), other)[0] for acc, m in mods.items()}
    assert not torch.equal(again[False], outs[False][0])                 # rebuilt from the new matrices
    assert torch.equal(again[True], outs[True][0])                       # the cached tables of the first call (pre_compute)
    # under autograd, through the 1x1 depth_net
    xg = x.to(DEV).requires_grad_(True)
    bev, _ = mods[False](xg, inp["img_metas"])
    bev.square().sum().backward()
    assert xg.grad is not None and xg.grad.abs().sum() > 0 and mods[False].depth_net.weight.grad.abs().sum() > 0
    cpu = LV.LSSViewTransformer_racformer(inp["grid_config"], inp["input_size"], downsample=inp["downsample"], in_channels=16,
                                          out_channels=c)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        cpu(x, inp["img_metas"])
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        LV.lss_view_transform(rig.logits, rig.feat(c), rig.m, LV.FrustumTables(*rig.axes), rig.grid, rig.batch)
