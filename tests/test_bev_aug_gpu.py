"""``rac_bev_aug_fwd`` (csrc/bev_aug.hip) against ``bev_aug.bev_aug_torch``, bit for bit, on the smallest shapes at which the kernel
can go wrong -- rows around the wave (63, 64, 65) and the chunk (255, 256, 257, and 513: three chunks), 3 / 5 / 7 columns, box sets
of 7 and 9 columns, empty segments first, last and in between, two samples with different draws in one table, bases one float off
every 16-byte boundary, in place, rows of NaN / inf / -0.0 / denormals --, its canaries, its repeatability, its capture into a graph,
and ``RaCFormer.prepare_bev_aug`` in front of the detector's built maps and ``forward_train``.

Bits are compared as integers with every NaN mapped to one pattern: which payload a NaN result carries is the hardware's choice and no
part of the rule; the columns that are only copied are compared raw."""
import numpy as np
import pytest
import torch

import detector_ref as DR
import detector_train_ref as TR
from racformer_amd import bev_aug as A, image_geom as G, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAP = 64                                    # untouched floats around every destination
SENTINEL = 0x7fa5a5a5                       # a NaN no computation produces
DRAWS = [A.BevDraw(0.3925, 1.05), A.BevDraw(-0.3011, 0.9502)]
ROWS = [0, 1, 63, 64, 65, A.CHUNK - 1, A.CHUNK, A.CHUNK + 1, 2 * A.CHUNK + 1]


def canon(t):
    """int32 bits, NaNs as one pattern"""
    t = t.detach().cpu().contiguous()
    return torch.where(t.isnan(), torch.tensor(0x7fc00000, dtype=torch.int32), t.view(torch.int32))


def raw(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def rows_of(n, cols, seed, special=True):
    """float32 [n, cols]: seeded values and, sprinkled over every column, NaN, +-inf, -0.0, +0.0 and denormals."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(n, cols, generator=g) * 20
    if special and n:
        vals = torch.tensor([float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 1e-41, -3e-39, 1.1754942e-38])
        where = torch.rand(n, cols, generator=g) < 0.15
        t[where] = vals[torch.randint(0, len(vals), (int(where.sum()),), generator=g)]
    return t


def spec_all(cols):
    """(rows, cols, kind, sample): an empty first and last segment, every row count at ``cols`` columns, both box widths."""
    spec = [(0, cols, "points", 0)]
    spec += [(n, cols, "points", i % 2) for i, n in enumerate(ROWS)]
    spec += [(n, w, "boxes", (i + j) % 2) for i, n in enumerate((0, 1, 5)) for j, w in enumerate((7, 9))]
    spec += [(A.CHUNK + 3, 9, "boxes", 1), (0, 9, "boxes", 0)]
    return spec


def arena(spec, shift, seed):
    """One float32 device buffer holding every segment of ``spec`` with ``GAP`` floats before, between and after, the first at
    ``shift`` floats from the (256-byte aligned) base and the next ones wherever the row lengths put them -> (buffer, views)."""
    total = shift + GAP + sum(n * c + GAP + 1 for n, c, _, _ in spec)
    buf = torch.full((total,), SENTINEL, dtype=torch.int32).view(torch.float32)
    at, views, host = shift + GAP, [], buf.clone()
    for i, (n, c, _, _) in enumerate(spec):
        if seed is not None:
            host[at:at + n * c] = rows_of(n, c, seed + i).flatten()
        views.append((at, n, c))
        at += n * c + GAP + 1                                      # (+ 1: the offsets walk through every residue mod 4)
    dev = host.to(DEV)
    return dev, [dev[a:a + n * c].view(n, c) for a, n, c in views]


def expected(srcs, spec, draws, device="cpu"):
    return [A.bev_aug_torch(s.to(device), A.draw_row(draws[b]), kind) for s, (_, _, kind, b) in zip(srcs, spec)]


def launch(spec, srcs, dsts, draws=DRAWS):
    plan = A.BevAugPlan([(s, d, kind, b) for s, d, (_, _, kind, b) in zip(srcs, dsts, spec)], len(draws))
    plan.launch(A.draw_table(draws, DEV))
    torch.cuda.synchronize()
    return plan


# ------------------------------------------------------------------------------------------------------------ the C-ABI
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("cols", [3, 5, 7])
def test_every_shape_bit_for_bit_with_canaries(cols, shift):
    spec = spec_all(cols)
    src_buf, srcs = arena(spec, shift, seed=100 * cols)
    dst_buf, dsts = arena(spec, 1 - shift, seed=None)                       # (sources and destinations one float apart mod 4)
    before = raw(src_buf)
    plan = launch(spec, srcs, dsts)
    assert plan.n_segs == len(spec) and plan.n_chunks == sum(-(-n // A.CHUNK) for n, _, _, _ in spec)
    want_cpu = expected([s.cpu() for s in srcs], spec, DRAWS)
    want_dev = expected(srcs, spec, DRAWS, DEV)
    for d, wc, wd, s, (n, c, kind, _) in zip(dsts, want_cpu, want_dev, srcs, spec):
        assert torch.equal(canon(d), canon(wc)) and torch.equal(canon(d), canon(wd)), f"{kind} {n} x {c}"
        copied = slice(3, None) if kind == "points" else slice(c, None)
        assert torch.equal(raw(d[:, copied]), raw(s[:, copied]))
    assert torch.equal(raw(src_buf), before)                                # the sources are only read
    written = torch.zeros(dst_buf.numel(), dtype=torch.bool)
    base = dst_buf.data_ptr()
    for d in dsts:
        a = (d.data_ptr() - base) // 4
        written[a:a + d.numel()] = True
    assert bool((raw(dst_buf)[~written] == SENTINEL).all())                 # GAP floats around every destination, and all the rest
    assert int((~written).sum()) >= GAP * (len(spec) + 1)
    # the special values did occur, on both sides of the rule
    allsrc = torch.cat([s.cpu().flatten() for s in srcs])
    assert bool(allsrc.isnan().any()) and bool(allsrc.isinf().any()) and bool(((allsrc != 0) & (allsrc.abs() < 1e-38)).any())
    assert bool((raw(allsrc) == -(2 ** 31)).any())                          # -0.0


def test_in_place_and_two_samples_in_one_table():
    spec = [(A.CHUNK + 7, 7, "points", 0), (A.CHUNK + 7, 7, "points", 1), (5, 9, "boxes", 1), (65, 5, "points", 0)]
    buf, views = arena(spec, 1, seed=7)
    srcs_cpu = [v.cpu().clone() for v in views]
    launch(spec, views, views)                                              # dst == src
    want = expected(srcs_cpu, spec, DRAWS)
    assert all(torch.equal(canon(v), canon(w)) for v, w in zip(views, want))
    # the two samples' draws differ, and each segment got its own
    same = rows_of(A.CHUNK + 7, 7, 9, special=False).to(DEV)
    out = [torch.empty_like(same), torch.empty_like(same)]
    launch(spec[:2], [same, same], out)
    assert not torch.equal(out[0], out[1])
    assert all(torch.equal(raw(o), raw(A.bev_aug_torch(same.cpu(), A.draw_row(DRAWS[b]), "points"))) for b, o in enumerate(out))


def test_repeatable_and_independent_of_the_address():
    spec = spec_all(5)
    _, srcs = arena(spec, 0, seed=31)
    _, d1 = arena(spec, 1, seed=None)
    _, d2 = arena(spec, 1, seed=None)
    launch(spec, srcs, d1)
    launch(spec, srcs, d2)
    _, srcs3 = arena(spec, 3, seed=31)                                      # the same rows elsewhere, at another residue mod 4
    _, d3 = arena(spec, 2, seed=None)
    launch(spec, srcs3, d3)
    for a, b, c in zip(d1, d2, d3):
        assert torch.equal(raw(a), raw(b)) and torch.equal(raw(a), raw(c))  # NaN payloads included


def test_captured_launch_takes_new_draws_from_the_table():
    spec = [(A.CHUNK + 1, 7, "points", 0), (40, 5, "points", 1), (5, 9, "boxes", 0), (0, 7, "points", 1)]
    _, srcs = arena(spec, 1, seed=50)
    _, dsts = arena(spec, 2, seed=None)
    plan = A.BevAugPlan([(s, d, kind, b) for s, d, (_, _, kind, b) in zip(srcs, dsts, spec)], 2)
    draws_a, draws_b = DRAWS, [A.BevDraw(0.05, 0.97), A.BevDraw(-0.2, 1.01)]
    table = A.draw_table(draws_a, DEV)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=torch.cuda.Stream()):
        plan.launch(table)
    for draws in (draws_b, draws_a):
        eager = [torch.empty_like(d) for d in dsts]
        launch(spec, srcs, eager, draws)
        table.copy_(A.draw_table(draws))
        for d in dsts:
            d.fill_(0)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(raw(d), raw(e)) for d, e in zip(dsts, eager))
        assert all(torch.equal(canon(d), canon(w)) for d, w in zip(dsts, expected([s.cpu() for s in srcs], spec, draws)))


def test_bad_tables_are_refused_before_the_launch():
    a, b = rows_of(10, 7, 1).to(DEV), torch.full((10, 7), 3.0, device=DEV)
    with pytest.raises(RuntimeError, match="overlap"):
        A.BevAugPlan([(a, b, "points", 0), (a, b, "points", 0)], 1).launch(A.draw_table(DRAWS[:1], DEV))      # two writers of b
    with pytest.raises(RuntimeError, match="overlap"):
        A.BevAugPlan([(a[:8], a[2:], "points", 0)], 1).launch(A.draw_table(DRAWS[:1], DEV))                   # neither apart nor in place
    plan = A.BevAugPlan([(a, b, "points", 0)], 1)
    plan.host[plan._chunk_at + 4] = 1                                       # the host copy's chunk now starts at row 1
    with pytest.raises(RuntimeError, match="chunk 0"):
        plan.launch(A.draw_table(DRAWS[:1], DEV))
    torch.cuda.synchronize()
    assert bool((b == 3.0).all())
    with pytest.raises(ValueError, match="draws table"):
        A.BevAugPlan([(a, b, "points", 0)], 1).launch(A.draw_table(DRAWS, DEV))
    with pytest.raises(ValueError, match="sample"):
        A.BevAugPlan([(a, b, "points", 1)], 1)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        A.BevAugPlan([(a.cpu(), b, "points", 0)], 1)


# ------------------------------------------------------------------------------------------------------------ the batch, the detector
def test_transform_batch_packs_like_pack_clouds():
    from racformer_amd.radar_pillars import pack_clouds
    T, B = 3, 2
    radar = [[rows_of(30 + 70 * t + 9 * b, 7, 60 + t + 5 * b) for b in range(B)] for t in range(T)]
    radar[1][1] = torch.zeros(0, 7)
    lidar = [rows_of(A.CHUNK * 2 + 5 + b, 5, 70 + b) for b in range(B)]
    boxes = [rows_of(5, 9, 80), torch.zeros(0, 9)]
    on = lambda xs: [x.to(DEV) for x in xs]                                 # noqa: E731
    r_dev, l_dev, b_dev = A.transform_batch([on(f) for f in radar], on(lidar), on(boxes), DRAWS)
    r_cpu, l_cpu, b_cpu = A.transform_batch(radar, lidar, boxes, DRAWS)
    for got, want in zip([r for f in r_dev for r in f] + l_dev + b_dev, [r for f in r_cpu for r in f] + l_cpu + b_cpu):
        assert got.is_cuda and got.shape == want.shape and torch.equal(canon(got), canon(want))
    # views into one packed tensor in pack_clouds' layout and order [b][t]: packing them again copies them as they lie
    packed, off = pack_clouds([r_dev[t][b] for b in range(B) for t in range(T)])
    assert r_dev[0][0].data_ptr() + 4 * packed.numel() == r_dev[T - 1][B - 1].data_ptr() + 4 * r_dev[T - 1][B - 1].numel()
    assert off.tolist() == np.cumsum([0] + [radar[t][b].shape[0] for b in range(B) for t in range(T)]).tolist()
    assert all(r_dev[t][b].is_contiguous() for t in range(T) for b in range(B))


def test_prepare_bev_aug_in_front_of_the_built_maps_and_forward_train():
    cfg = syn.SMALL
    det = DR.build(cfg).to(DEV)
    det.fused_grad = True
    det.train()
    a = TR.train_args(cfg, (3, 2), device=DEV)
    B, T, N = 2, cfg.num_frames, cfg.num_cams
    fH, fW = cfg.image_hw
    ida = G.RandomTransformImage(dict(H=150, W=400, final_dim=(fH, fW), resize_lim=(0.45, 0.6), bot_pct_lim=(0.0, 0.1), rot_lim=(0.0, 0.0),
                                      rand_flip=True), training=True)
    rawf = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (B, T * N, 150, 400, 3), dtype=np.uint8)).to(DEV)
    np.random.seed(21)
    img, metas = det.prepare_raw(rawf, a["img_metas"], ida)
    # lidar clouds as in the point-map tests: the samples' radar clouds of two frames, spread out
    clouds = [torch.cat([a["radar_points"][0][b][:, :5] * 3.0, a["radar_points"][1][b][:, :5] * 2.0]) for b in range(B)]
    bev = A.RaCGlobalRotScaleTransImage()
    draws = [bev.draw() for _ in range(B)]
    # the device route
    m_dev, r_dev, l_dev, b_dev = det.prepare_bev_aug(metas, a["radar_points"], clouds, a["gt_bboxes_3d"], transform=bev, draws=draws)
    # the host route: the reference's dict behaviour per sample on CPU tensors, then the uploads
    m_host, r_host, l_host, b_host = [], [[None] * B for _ in range(T)], [], []
    for b in range(B):
        res = dict(lidar2img=[np.array(m) for m in metas[b]["lidar2img"]], points=clouds[b].cpu(),
                   radar_points=[a["radar_points"][t][b].cpu() for t in range(T)], gt_bboxes_3d=a["gt_bboxes_3d"][b].cpu())
        bev(res, draw=draws[b])
        m_host.append(dict(metas[b], lidar2img=res["lidar2img"]))
        l_host.append(res["points"].to(DEV))
        b_host.append(res["gt_bboxes_3d"].to(DEV))
        for t in range(T):
            r_host[t][b] = res["radar_points"][t].to(DEV)
    assert all(np.array_equal(x, y) and x.dtype == y.dtype for b in range(B) for x, y in zip(m_dev[b]["lidar2img"], m_host[b]["lidar2img"]))
    assert all(torch.equal(raw(x), raw(y)) for x, y in zip(b_dev, b_host)) and all(x.shape == (n, 9) for x, n in zip(b_dev, (3, 2)))
    pad_hw = tuple(a["gt_depth"].shape[-2:])
    maps_dev = det.point_maps(img, r_dev, m_dev) + (det.lidar_gt_depth(l_dev, img, m_dev, pad_hw=pad_hw),)
    maps_host = det.point_maps(img, r_host, m_host) + (det.lidar_gt_depth(l_host, img, m_host, pad_hw=pad_hw),)
    for x, y in zip(maps_dev, maps_host):
        assert x.count_nonzero() > 0 and torch.equal(raw(x), raw(y))
    # (the views turn with the scene, so the maps barely change; the clouds and the caller's inputs tell that something happened)
    assert not torch.equal(r_dev[0][0], a["radar_points"][0][0]) and r_dev[0][0].shape == a["radar_points"][0][0].shape
    TR.seed_all(5)
    losses = det.forward_train(img_metas=m_dev, gt_bboxes_3d=b_dev, gt_labels_3d=a["gt_labels_3d"], gt_depth=None, img=img,
                               radar_points=r_dev, radar_depth=None, radar_rcs=None, points=l_dev)
    L = cfg.num_layers
    want_keys = {"loss_depth", "loss_cls", "loss_bbox"} | {f"d{i}.loss_{k}" for i in range(L - 1) for k in ("cls", "bbox")}
    want_keys |= {k + "_dn" for k in want_keys if k != "loss_depth"}
    assert set(losses) == want_keys
    assert all(v.dim() == 0 and v.is_cuda and bool(torch.isfinite(v)) for v in losses.values()) and float(losses["loss_depth"]) > 0
