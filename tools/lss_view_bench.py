#!/usr/bin/env python3
"""Timing of the Lift-Splat view transform (racformer_amd/lss_view.py) on the f8 shape: 6 cameras, D = 96, a 16 x 44 feature
map, C = 256, a 128 x 128 grid of 0.8 m cells, the reference's frustum (synthetic.make_lss_view_inputs).  Needs the GPU.

    python tools/lss_view_bench.py [--out profiles/lss_view_f8.json] [--errors lss_view_errors.json]

Three records, all between device events on one stream after a warm-up, medians over --reps calls, the two routes alternating:
  kernels   every rac_lss_* entry point alone
  operator  the fused operator: forward with the tables rebuilt (accelerate=False), forward on cached tables, forward + backward;
            beside it the route a user has without it -- torch ops on the GPU for the preparation (broadcast matmul, the three
            mask compactions, argsort, where: the reference's steps), softmax, the permutes, and bev_pool_v2 for the splat
            and its backward
  long_cell rac_bev_pool_v2_fwd alone on the reference frustum's tables (fullest cell 4 416 points) against
            synthetic.make_lss_ranks' tables (416), same C
--errors: the (E_ref, kernel error) pairs a `RAC_LSS_VIEW_ERRORS=<file> pytest -m gpu tests/test_lss_view_gpu.py` session wrote,
copied into the record.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from racformer_amd import _lib, lss_view as LV, synthetic as syn  # noqa: E402
from racformer_amd.bev_pool import QuickCumsumCuda, bev_pool_v2, intervals_from_ranks  # noqa: E402


def timed(fns, reps, warmup=5):
    """{name: median ms}; the functions alternate inside every repetition"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ev = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    return {k: round(statistics.median(a.elapsed_time(b) for a, b in v), 4) for k, v in ev.items()}


def torch_prepare(m, frustum, lower, interval, size, B, N):
    """voxel_pooling_prepare_v2 over get_lidar_coor in torch ops on the GPU: the reference's steps, host syncs included"""
    D, H, W, _ = frustum.shape
    coords = torch.cat((frustum, torch.ones_like(frustum[..., :1])), -1)
    coords[..., :2] = coords[..., :2] * torch.maximum(coords[..., 2:3], torch.ones_like(coords[..., 2:3]) * 1e-5)
    coords = coords.view(1, 1, D, H, W, 4, 1).repeat(B, N, 1, 1, 1, 1, 1)
    mm = m.view(B, N, 1, 1, 1, 4, 4).repeat(1, 1, D, H, W, 1, 1)
    coor = torch.matmul(mm, coords).squeeze(-1)[..., :3]
    n = B * N * D * H * W
    ranks_depth = torch.arange(0, n, dtype=torch.int, device=m.device)
    ranks_feat = torch.arange(0, n // D, dtype=torch.int, device=m.device).reshape(B, N, 1, H, W).expand(B, N, D, H, W).flatten()
    coor = ((coor - lower) / interval).long().view(n, 3)
    batch_idx = torch.arange(0, B, device=m.device).reshape(B, 1).expand(B, n // B).reshape(n, 1)
    coor = torch.cat((coor, batch_idx), 1)
    kept = (coor[:, 0] >= 0) & (coor[:, 0] < size[0]) & (coor[:, 1] >= 0) & (coor[:, 1] < size[1]) & (coor[:, 2] >= 0) & \
        (coor[:, 2] < size[2])
    coor, ranks_depth, ranks_feat = coor[kept], ranks_depth[kept], ranks_feat[kept]
    ranks_bev = coor[:, 3] * (size[2] * size[1] * size[0]) + coor[:, 2] * (size[1] * size[0]) + coor[:, 1] * size[0] + coor[:, 0]
    order = ranks_bev.argsort()
    ranks_bev, ranks_depth, ranks_feat = ranks_bev[order], ranks_depth[order], ranks_feat[order]
    first = torch.ones(ranks_bev.shape[0], device=m.device, dtype=torch.bool)
    first[1:] = ranks_bev[1:] != ranks_bev[:-1]
    starts = torch.where(first)[0].int()
    lengths = torch.zeros_like(starts)
    lengths[:-1] = starts[1:] - starts[:-1]
    lengths[-1] = ranks_bev.shape[0] - starts[-1]
    return ranks_bev.int().contiguous(), ranks_depth.int().contiguous(), ranks_feat.int().contiguous(), starts, lengths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "lss_view_f8.json"))
    ap.add_argument("--errors", default=None)
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lss_view_bench needs the MI355X"
    dev = "cuda:0"
    C = 256
    inp = syn.make_lss_view_inputs(channels=C)
    mod = LV.LSSViewTransformer_racformer(inp["grid_config"], inp["input_size"], inp["downsample"], in_channels=16,
                                          out_channels=C).to(dev)
    B, N = len(inp["img_metas"]), len(inp["img_metas"][0]["lidar2img"])
    logits, feat = inp["depth_digit"].to(dev), inp["tran_feat"].to(dev)
    shape = tuple(logits.shape)
    bn, D, H, W = shape
    grid, X, Y, Z = mod.grid, *mod.grid.size
    tabs = LV.FrustumTables(mod.depth_table, mod.v_table, mod.u_table)
    m = LV.img2lidar_from_metas(inp["img_metas"]).to(dev)
    ranks = LV.lss_rank_tables(m, tabs, grid, B, shape)
    n_kept, n_occ = (int(v) for v in ranks.counts.cpu())
    fullest = int(ranks.interval_lengths.max())
    gout = torch.randn(B, Z * C, Y, X, device=dev)
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream_ptr
    n_points, n_cells = bn * D * H * W, B * X * Y * Z

    # ---- every entry point alone
    cells = ranks.cells
    work = torch.empty(3 * n_cells + n_points, dtype=torch.int32, device=dev)
    stats = torch.empty(bn * H * W, 2, device=dev)
    feat_cl = torch.empty(bn * H * W * C, device=dev)
    cell_interval = torch.empty(n_cells, dtype=torch.int32, device=dev)
    partial = torch.empty((-(-n_points // LV.LSS_CHUNK) + min(n_points, n_cells)) * C, device=dev)
    out = torch.empty(B, Z * C, Y, X, device=dev)
    grad_cell, gfeat_cl, gfeat, glog = torch.empty(n_cells * C, device=dev), torch.empty_like(feat_cl), torch.empty_like(feat), \
        torch.empty_like(logits)
    (lx, ly, lz), (ix, iy, iz) = grid.lower, grid.interval
    kernels = timed({
        "rac_lss_cells_fwd": lambda: L.rac_lss_cells_fwd(p(m), p(tabs.depth), p(tabs.v), p(tabs.u), p(cells), bn, N, D, H, W, lx, ly,
                                                         lz, ix, iy, iz, X, Y, Z, st()),
        "rac_lss_tables_fwd": lambda: L.rac_lss_tables_fwd(p(cells), p(ranks.ranks_bev), p(ranks.ranks_depth), p(ranks.ranks_feat),
                                                           p(ranks.interval_starts), p(ranks.interval_lengths), p(ranks.counts),
                                                           p(work), n_points, n_cells, D, H * W, st()),
        "rac_lss_softmax_stats_fwd": lambda: L.rac_lss_softmax_stats_fwd(p(logits), p(stats), bn, D, H * W, st()),
        "rac_lss_transpose_fwd(feat)": lambda: L.rac_lss_transpose_fwd(p(feat), p(feat_cl), bn, C, H * W, st()),
        "rac_lss_splat_fwd": lambda: L.rac_lss_splat_fwd(p(logits), p(stats), p(feat_cl), p(ranks.ranks_depth), p(ranks.ranks_feat),
                                                         p(ranks.ranks_bev), p(ranks.interval_starts), p(ranks.interval_lengths),
                                                         p(ranks.counts), p(cell_interval), p(partial), p(out), n_points, B, C, X, Y,
                                                         Z, st()),
        "rac_lss_transpose_fwd(grad)": lambda: L.rac_lss_transpose_fwd(p(gout), p(grad_cell), B * Z, C, Y * X, st()),
        "rac_lss_view_bwd": lambda: L.rac_lss_view_bwd(p(grad_cell), p(logits), p(stats), p(feat_cl), p(cells), p(gfeat_cl), p(glog),
                                                       bn, C, D, H * W, st()),
        "rac_lss_transpose_fwd(grad_feat)": lambda: L.rac_lss_transpose_fwd(p(gfeat_cl), p(gfeat), bn, H * W, C, st()),
    }, args.reps)

    # ---- the operator against the route without it
    lg, ft = logits.clone().requires_grad_(True), feat.clone().requires_grad_(True)
    lower = torch.tensor(grid.lower, device=dev)
    interval = torch.tensor(grid.interval, device=dev)
    size = torch.tensor([float(v) for v in grid.size], device=dev)
    frustum = mod.frustum.data

    def torch_forward(tables, a=logits, f=feat):
        rb, rd, rf, gs, gl = tables
        depth = a.softmax(dim=1).view(B, N, D, H, W)
        fl = f.view(B, N, C, H, W).permute(0, 1, 3, 4, 2)
        o = bev_pool_v2(depth, fl, rd, rf, rb, (B, Z, Y, X, C), gs, gl)
        return torch.cat(o.unbind(dim=2), 1)

    tt = torch_prepare(m, frustum, lower, interval, size, B, N)
    ours, theirs = LV.lss_view_transform(logits, feat, m, tabs, grid, B, ranks=ranks), torch_forward(tt)
    agree = (ours - theirs).abs().max().item()

    def fused_train():
        o = LV.lss_view_transform(lg, ft, m, tabs, grid, B)
        torch.autograd.grad(o, (lg, ft), gout)

    def torch_train():
        o = torch_forward(torch_prepare(m, frustum, lower, interval, size, B, N), lg, ft)
        torch.autograd.grad(o, (lg, ft), gout)

    operator = timed({
        "fused_forward_tables_rebuilt": lambda: LV.lss_view_transform(logits, feat, m, tabs, grid, B),
        "torch_forward_tables_rebuilt": lambda: torch_forward(torch_prepare(m, frustum, lower, interval, size, B, N)),
        "fused_tables_only": lambda: LV.lss_rank_tables(m, tabs, grid, B, shape),
        "torch_tables_only": lambda: torch_prepare(m, frustum, lower, interval, size, B, N),
        "fused_forward_cached_tables": lambda: LV.lss_view_transform(logits, feat, m, tabs, grid, B, ranks=ranks),
        "torch_forward_cached_tables": lambda: torch_forward(tt),
        "fused_forward_backward_tables_rebuilt": fused_train,
        "torch_forward_backward_tables_rebuilt": torch_train,
    }, max(args.reps // 4, 10))

    # ---- the long cell in the existing pooling kernel
    depth = logits.softmax(dim=1).contiguous()
    fl = feat.view(B, N, C, H, W).permute(0, 1, 3, 4, 2).contiguous()
    syn_rd, syn_rf, syn_rb = (t.to(dev) for t in syn.make_lss_ranks(N, D, H, W, X))
    syn_gs, syn_gl = intervals_from_ranks(syn_rb)
    shape5 = (B, Z, Y, X, C)
    ref_t = (ranks.ranks_bev[:n_kept], ranks.ranks_depth[:n_kept], ranks.ranks_feat[:n_kept], ranks.interval_starts[:n_occ],
             ranks.interval_lengths[:n_occ])
    long_cell = timed({
        "bev_pool_v2_fwd_reference_frustum": lambda: QuickCumsumCuda.apply(depth, fl, ref_t[1], ref_t[2], ref_t[0], shape5, ref_t[3],
                                                                           ref_t[4]),
        "bev_pool_v2_fwd_make_lss_ranks": lambda: QuickCumsumCuda.apply(depth, fl, syn_rd, syn_rf, syn_rb, shape5, syn_gs, syn_gl),
    }, args.reps)
    long_cell.update(reference_frustum=dict(points=n_kept, cells=n_occ, fullest_cell=fullest),
                     make_lss_ranks=dict(points=int(syn_rd.numel()), cells=int(syn_gs.numel()), fullest_cell=int(syn_gl.max())))

    rec = dict(shape=dict(cams=N, D=D, H=H, W=W, C=C, grid=[X, Y, Z], points=n_points, kept=n_kept, occupied_cells=n_occ,
                          fullest_cell=fullest),
               device=torch.cuda.get_device_name(0), unit="ms, median of device-event times", reps=args.reps,
               kernels=kernels, operator=operator, fused_vs_torch_max_abs_diff=agree, long_cell=long_cell)
    if args.errors and os.path.exists(args.errors):
        rec["tolerance_bases"] = json.load(open(args.errors))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
