"""The BEV augmentation on the host (racformer_amd/bev_aug.py): the reference's draws, matrices and order of calls from the fixture
``tests/golden/bev_aug_small.npz`` (written by the reference's own ``RaCGlobalRotScaleTransImage.__call__``), the direction of the
rotation and the sign of the yaw by a float64 property that separates right from wrong, the accuracy of the float32 rule against the
same rule in float64, its quirks, the two annotation filters and the dict behaviour.  No GPU."""
import os

import numpy as np
import pytest
import torch

from racformer_amd import bev_aug as A

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24
GAMMA3 = 3 * U / (1 - 3 * U)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "bev_aug_small.npz"))
    cases = {}
    for key in z.files:
        name, field = key.split(":")
        cases.setdefault(name, {})[field] = z[key]
    assert sorted(cases) == ["a", "b", "c"]
    return cases


def transform_of(c):
    return A.RaCGlobalRotScaleTransImage(rot_range=c["rot_range"].tolist(), scale_ratio_range=c["scale_ratio_range"].tolist())


def draw_of(c):
    return A.BevDraw(float(c["draws"][0]), float(c["draws"][1]))


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous().view(torch.int64)


# ------------------------------------------------------------------------------------------------------------ the fixture
def test_draws_are_the_references(golden):
    for c in golden.values():
        np.random.seed(int(c["seed"]))
        d = transform_of(c).draw()
        assert (d.rot_angle, d.scale_ratio) == tuple(c["draws"].tolist())
        after = np.random.rand()
        np.random.seed(int(c["seed"]))
        np.random.uniform(0, 1), np.random.uniform(0, 1)
        assert np.random.rand() == after                    # exactly two draws


def test_view_mats_are_the_references_bit_for_bit(golden):
    for c in golden.values():
        got = A.view_mats(list(c["lidar2img_in"]), draw_of(c))
        want = c["lidar2img_out"]
        assert want.dtype == np.float32 and len(got) == len(want) == 8
        for g, w in zip(got, want):
            assert g.dtype == np.float32 and np.array_equal(g.view(np.int32), w.view(np.int32))


class Holder:
    """An object with ``.tensor``, as the reference's clouds and boxes are."""

    def __init__(self, tensor):
        self.tensor = tensor


def results_of(c, holders=False):
    """Results with the fixture case's keys, by the names of its call log."""
    keys = list(dict.fromkeys(c["log_key"].tolist()))
    g = torch.Generator().manual_seed(3)
    res, named = dict(lidar2img=[m.copy() for m in c["lidar2img_in"]]), {}
    for key in keys:
        t = torch.randn(4, 9 if key.startswith("gt_") else (7 if key.startswith("radar") else 5), generator=g)
        named[key] = Holder(t) if holders else t
        if key.startswith("radar_points["):
            res.setdefault("radar_points", []).append(named[key])
        else:
            res[key] = named[key]
    return res, named


def test_call_touches_the_keys_in_the_references_order(golden, monkeypatch):
    for c in golden.values():
        res, named = results_of(c, holders=True)
        names = {id(h.tensor): k for k, h in named.items()}
        log = []

        def recorder(op, fn):
            def wrapped(t, value):
                out = fn(t, value)
                log.append((names.pop(id(t)), op, value))
                names[id(out)] = log[-1][0]
                return out
            return wrapped

        for op, kinds in (("rotate", ("rotate_points", "rotate_boxes")), ("scale", ("scale_points", "scale_boxes"))):
            for fn in kinds:
                monkeypatch.setattr(A, fn, recorder(op, getattr(A, fn)))
        out = transform_of(c)(res, draw=draw_of(c))
        monkeypatch.undo()
        assert out is res
        assert [e[0] for e in log] == c["log_key"].tolist() and [e[1] for e in log] == c["log_op"].tolist()
        assert [e[2] for e in log] == c["log_val"].tolist()                     # the angle and the ratio as drawn, unrounded
        # the reference rotates about axis 2 where it names an axis (the clouds) and leaves the boxes' default, which is z as well
        assert set(c["log_axis"][[k.startswith("gt_") for k in c["log_key"]]].tolist()) == {-1}
        assert set(c["log_axis"][[not k.startswith("gt_") and op == "rotate" for k, op in zip(c["log_key"], c["log_op"])]].tolist()) <= {2}
        for g, w in zip(res["lidar2img"], c["lidar2img_out"]):
            assert np.array_equal(g.view(np.int32), w.view(np.int32))
        for key, h in named.items():                                            # the objects keep their identity, the rows are the rule's
            kind = "boxes" if key.startswith("gt_") else "points"
            first = results_of(c)[1][key]
            assert torch.equal(bits(h.tensor), bits(A.bev_aug_torch(first, A.draw_row(draw_of(c)), kind)))


# ------------------------------------------------------------------------------------------------------------ direction
def camera(hw, yaw, t):
    """float64 lidar2img of a pinhole camera at ``t`` looking along the lidar frame's x axis turned by ``yaw`` (90 degrees wide)."""
    H, W = hw
    f = W / 2.0
    K = np.array([[f, 0, W / 2.0], [0, f, H / 2.0], [0, 0, 1.0]])
    c, s = np.cos(yaw), np.sin(yaw)
    fwd, left, up = np.array([c, s, 0.0]), np.array([-s, c, 0.0]), np.array([0.0, 0.0, 1.0])
    R = np.stack([-left, -up, fwd])
    M = np.eye(4)
    M[:3, :3] = K @ R
    M[:3, 3] = -K @ R @ np.asarray(t, np.float64)
    return M


def corners(box):
    """The eight corners [n, 8, 3] of float64 boxes (bottom centre, w along the box's x, yaw counter-clockwise about z)."""
    sx = torch.tensor([0.5, 0.5, -0.5, -0.5] * 2, dtype=box.dtype)
    sy = torch.tensor([0.5, -0.5, -0.5, 0.5] * 2, dtype=box.dtype)
    sz = torch.tensor([0.0] * 4 + [1.0] * 4, dtype=box.dtype)
    lx, ly, lz = box[:, 3:4] * sx, box[:, 4:5] * sy, box[:, 5:6] * sz
    cy, sn = torch.cos(box[:, 6:7]), torch.sin(box[:, 6:7])
    return torch.stack([box[:, 0:1] + lx * cy - ly * sn, box[:, 1:2] + lx * sn + ly * cy, box[:, 2:3] + lz], dim=2)


def homogeneous(M, p):
    """(M [p, 1], sum_j |M_ij p_j|) for float64 M [4, 4] and points [n, 3]."""
    ph = torch.cat([p, torch.ones(len(p), 1, dtype=p.dtype)], dim=1)
    return ph @ M.T, ph.abs() @ M.abs().T


@pytest.mark.parametrize("angle, ratio", [(0.3925, 1.05), (-0.3925, 0.95), (0.11, 1.0), (2.5, 0.7)])
def test_direction_of_the_rotation_and_sign_of_the_yaw(angle, ratio):
    g = torch.Generator().manual_seed(7)
    draw = A.BevDraw(angle, ratio)
    row = A.draw_row(draw)
    mats = [camera((256, 704), yaw, (0.5, 0.1 * i, 1.6)) for i, yaw in enumerate((0.0, 1.3, 3.0, -2.0))]
    new = A.view_mats(mats, draw)
    pts = torch.cat([torch.rand(64, 2, generator=g, dtype=torch.float64) * 100 - 50, torch.rand(64, 1, generator=g, dtype=torch.float64) * 6 - 3], 1)
    box = torch.cat([torch.rand(16, 2, generator=g, dtype=torch.float64) * 100 - 50, torch.rand(16, 1, generator=g, dtype=torch.float64) * 2 - 2,
                     torch.rand(16, 3, generator=g, dtype=torch.float64) * 4 + 0.5, torch.rand(16, 1, generator=g, dtype=torch.float64) * 6.28 - 3.14,
                     torch.rand(16, 2, generator=g, dtype=torch.float64) * 20 - 10], 1)
    pts2 = A.bev_aug_torch(pts, row, "points")
    box2 = A.bev_aug_torch(box, row, "boxes")
    for M, M2 in zip(mats, new):
        M, M2 = torch.from_numpy(M), torch.from_numpy(M2.astype(np.float64))
        for before, after in ((pts, pts2), (corners(box).reshape(-1, 3), corners(box2).reshape(-1, 3))):
            want, _ = homogeneous(M, before)
            got, scale = homogeneous(M2, after)
            assert bool(((got - want).abs() <= 1e-5 * scale).all())
    # a box's corners from (centre', dims', yaw') are the transformed corners of the input box
    moved = A.bev_aug_torch(corners(box).reshape(-1, 3), row, "points").reshape(-1, 8, 3)
    built = corners(box2)
    scale = (box2[:, :3].abs().sum(1) + box2[:, 3:6].abs().sum(1))[:, None, None]      # the terms a corner is summed from
    assert bool(((built - moved).abs() <= 1e-5 * scale).all())
    # the velocity turns and grows as a displacement does: the image of p + v minus the image of p
    tip = A.bev_aug_torch(torch.cat([box[:, :2] + box[:, 7:9], box[:, 2:3]], 1), row, "points")
    disp = tip[:, :2] - box2[:, :2]
    assert bool(((box2[:, 7:9] - disp).abs() <= 1e-5 * (tip[:, :2].abs() + box2[:, :2].abs())).all())
    # and the property does tell: the other sense of rotation, or no scaling, misses by far
    wrong = A.bev_aug_torch(pts, A.draw_row(A.BevDraw(-angle, ratio)), "points")
    want, _ = homogeneous(torch.from_numpy(mats[0]), pts)
    got, scale = homogeneous(torch.from_numpy(new[0].astype(np.float64)), wrong)
    assert not bool(((got - want).abs() <= 1e-5 * scale).all())


# ------------------------------------------------------------------------------------------------------------ accuracy
def magnitudes(n, cols, seed):
    """float32 [n, cols] of either sign with magnitudes log-uniform in [1e-3, 1e3]."""
    g = torch.Generator().manual_seed(seed)
    mag = 10.0 ** (torch.rand(n, cols, generator=g, dtype=torch.float64) * 6 - 3)
    return (mag * (torch.randint(0, 2, (n, cols), generator=g) * 2 - 1)).float()


@pytest.mark.parametrize("angle, ratio", [(0.3925, 1.05), (-0.2, 0.95), (1e-3, 1.0), (3.0, 1.2)])
def test_float32_rule_against_float64(angle, ratio):
    row = A.draw_row(A.BevDraw(angle, ratio))
    c, s, _, r = (abs(float(v)) for v in row)
    for kind, t in (("points", magnitudes(512, 7, 1)), ("boxes", magnitudes(512, 9, 2))):
        got = A.bev_aug_torch(t, row, kind).double()
        want = A.bev_aug_torch(t.double(), row, kind)
        assert got.dtype == want.dtype == torch.float64
        a = t.double().abs()
        bound = {0: (a[:, 0] * c + a[:, 1] * s) * r, 1: (a[:, 0] * s + a[:, 1] * c) * r, 2: a[:, 2] * r}
        if kind == "boxes":
            bound.update({7: (a[:, 7] * c + a[:, 8] * s) * r, 8: (a[:, 7] * s + a[:, 8] * c) * r, 3: a[:, 3] * r, 4: a[:, 4] * r, 5: a[:, 5] * r,
                          6: a[:, 6] + abs(float(row[2]))})
        for col, b in bound.items():
            err = (got[:, col] - want[:, col]).abs()
            assert bool((err <= GAMMA3 * b).all()), f"{kind} column {col}: {float((err / b).max()) / U:.3f} u"
        rest = [k for k in range(t.shape[1]) if k not in bound]
        assert torch.equal(bits(A.bev_aug_torch(t, row, kind)[:, rest]), bits(t[:, rest]))


# ------------------------------------------------------------------------------------------------------------ quirks
ROW = A.draw_row(A.BevDraw(0.3, 1.04))


def test_radar_columns_from_3_on_are_copied_bit_for_bit():
    t = magnitudes(33, 7, 4)
    t[0, 3:] = torch.tensor([float("nan"), float("inf"), -0.0, 1e-41])
    t.view(torch.int32)[1, 4] = 0x7fc12345                 # a NaN with a payload
    out = A.bev_aug_torch(t, ROW, "points")
    assert torch.equal(bits(out[:, 3:]), bits(t[:, 3:]))   # the velocity columns 4 and 5 included: neither turned nor scaled
    assert not torch.equal(out[:, :3], t[:, :3])


def test_nan_and_inf_spread_as_through_a_matmul():
    t = torch.ones(3, 5)
    t[0, 2] = float("nan")
    t[1, 0] = float("inf")
    t[2, 1] = float("-inf")
    out = A.bev_aug_torch(t, ROW, "points")
    assert bool(out[0, :3].isnan().all())                  # a NaN z makes x' and y' NaN
    assert bool(out[1, 2].isnan()) and bool(out[1, :2].isinf().all())       # an inf x makes z' NaN (inf times 0)
    assert bool(out[2, 2].isnan())
    assert torch.equal(out[:, 3:], t[:, 3:])


def test_seven_column_boxes_and_empty_inputs():
    b9 = magnitudes(5, 9, 6)
    out7, out9 = A.bev_aug_torch(b9[:, :7].contiguous(), ROW, "boxes"), A.bev_aug_torch(b9, ROW, "boxes")
    assert out7.shape == (5, 7) and torch.equal(bits(out7), bits(out9[:, :7]))
    assert torch.equal(out9[:, 6], b9[:, 6] + torch.tensor(float(ROW[2])))           # yaw + a, not re-limited
    assert A.bev_aug_torch(torch.zeros(0, 7), ROW, "points").shape == (0, 7)
    assert A.bev_aug_torch(torch.zeros(0, 9), ROW, "boxes").shape == (0, 9)
    with pytest.raises(ValueError, match="7 or 9"):
        A.bev_aug_torch(torch.zeros(2, 8), ROW, "boxes")
    radar, points, boxes = A.transform_batch([[torch.zeros(0, 7)]], [torch.zeros(0, 5)], [torch.zeros(0, 9)], [A.BevDraw(0.1, 1.0)])
    assert radar[0][0].shape == (0, 7) and points[0].shape == (0, 5) and boxes[0].shape == (0, 9)


def test_transform_batch_on_cpu_is_the_rule_per_sample():
    T, B = 3, 2
    radar = [[magnitudes(5 + t + 4 * b, 7, 10 + t + 3 * b) for b in range(B)] for t in range(T)]
    lidar = [magnitudes(40 + b, 5, 20 + b) for b in range(B)]
    boxes = [magnitudes(3, 9, 30), torch.zeros(0, 9)]
    draws = [A.BevDraw(0.2, 1.03), A.BevDraw(-0.3, 0.96)]
    keep = [r.clone() for frame in radar for r in frame]
    r2, l2, b2 = A.transform_batch(radar, lidar, boxes, draws)
    for b in range(B):
        row = A.draw_row(draws[b])
        for t in range(T):
            assert torch.equal(bits(r2[t][b]), bits(A.bev_aug_torch(radar[t][b], row, "points")))
        assert torch.equal(bits(l2[b]), bits(A.bev_aug_torch(lidar[b], row, "points")))
        assert torch.equal(bits(b2[b]), bits(A.bev_aug_torch(boxes[b], row, "boxes")))
    assert all(torch.equal(a, b) for a, b in zip(keep, [r for frame in radar for r in frame]))      # the caller's clouds stay
    # views into packed tensors, the radar clouds sample-major
    assert r2[1][0].data_ptr() == r2[0][0].data_ptr() + 4 * r2[0][0].numel() and r2[0][1].data_ptr() == r2[2][0].data_ptr() + 4 * r2[2][0].numel()
    r3, l3, b3 = A.transform_batch(radar, None, None, draws)
    assert l3 is None and b3 is None and torch.equal(r3[2][1], r2[2][1])
    with pytest.raises(ValueError, match="samples"):
        A.transform_batch(radar, lidar[:1], None, draws)


# ------------------------------------------------------------------------------------------------------------ the C-ABI's refusals
def test_c_abi_checks_the_host_tables_before_any_launch():
    """Every refusal of ``rac_bev_aug_fwd`` comes before its first HIP call, so it shows without a GPU (the addresses are never read)."""
    import ctypes
    from racformer_amd import _lib
    lib = _lib.lib()

    def call(segs, chunks, n_samples=1, n_chunks=None):
        seg = np.array(segs, A._SEG)
        chk = np.array(chunks, A._CHUNK) if chunks else np.zeros(1, A._CHUNK)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)                          # noqa: E731
        rc = lib.rac_bev_aug_fwd(p(seg), p(chk), p(seg), p(chk), ctypes.c_void_p(4096), len(seg), len(chunks) if n_chunks is None else n_chunks,
                                 n_samples, None)
        return rc, lib.rac_last_error().decode()

    src, dst = 1 << 20, 1 << 21
    assert call([(src, dst, 0, 7, A.POINTS, 0), (0, 0, 0, 9, A.BOXES, 0)], [])[0] == 0          # nothing to do: nothing is launched
    for segs, chunks, word in [
            ([(src, dst, 10, 2, A.POINTS, 0)], [(0, 0)], "columns"),
            ([(src, dst, 10, A.MAX_COLS + 1, A.POINTS, 0)], [(0, 0)], "columns"),
            ([(src, dst, 10, 8, A.BOXES, 0)], [(0, 0)], "columns"),
            ([(src, dst, 10, 7, 2, 0)], [(0, 0)], "kind"),
            ([(src, dst, -1, 7, A.POINTS, 0)], [], "rows"),
            ([(src, dst, 10, 7, A.POINTS, 1)], [(0, 0)], "sample"),
            ([(src, 0, 10, 7, A.POINTS, 0)], [(0, 0)], "null"),
            ([(src + 2, dst, 10, 7, A.POINTS, 0)], [(0, 0)], "misaligned"),
            ([(src, src + 28, 10, 7, A.POINTS, 0)], [(0, 0)], "overlaps"),                        # shifted by one row: not in place
            ([(src, dst, 10, 7, A.POINTS, 0), (dst + 28 * 9, dst + 4096, 10, 7, A.POINTS, 0)], [(0, 0), (1, 0)], "overlaps"),
            ([(src, dst, 10, 7, A.POINTS, 0), (src, dst + 28 * 9, 10, 7, A.POINTS, 0)], [(0, 0), (1, 0)], "overlap"),
            ([(src, dst, 300, 7, A.POINTS, 0)], [(0, 0)], "chunk"),                               # a row no chunk names
            ([(src, dst, 300, 7, A.POINTS, 0)], [(0, 0), (0, 255)], "chunk 1"),
            ([(src, dst, 10, 7, A.POINTS, 0)], [(0, 0), (0, 256)], "chunks"),                     # a chunk past the rows
    ]:
        rc, msg = call(segs, chunks)
        assert rc == -1 and word in msg, (segs, chunks, msg)
    assert call([(src, src, 10, 7, A.POINTS, 0)], [(0, 0)], n_samples=0)[0] == -1


# ------------------------------------------------------------------------------------------------------------ the filters
def test_range_filter_edges_and_yaw_wrap():
    f = A.ObjectRangeFilter([-51.2, -51.2, -5.0, 51.2, 51.2, 3.0])
    lo, hi, pi = float(np.float32(-51.2)), float(np.float32(51.2)), float(np.float32(np.pi))
    box = torch.zeros(8, 9)
    box[:, 0] = torch.tensor([0.0, lo, hi, 1.0, 1.0, 50.0, np.nextafter(np.float32(hi), np.float32(0)), -60.0])
    box[:, 1] = torch.tensor([0.0, 0.0, 0.0, lo, hi, -50.0, np.nextafter(np.float32(lo), np.float32(0)), 0.0])
    box[:, 2] = 100.0                                                           # z is not looked at
    box[:, 6] = torch.tensor([pi, 0, 0, 0, 0, -pi, 7.0, 0])
    box[:, 7] = torch.arange(8.0)
    labels = torch.arange(8)
    out, lab = f(box, labels)
    assert lab.tolist() == [0, 5, 6] and out[:, 7].tolist() == [0.0, 5.0, 6.0]          # a box exactly on lo or on hi is dropped; order kept
    assert out[0, 6].item() == -pi and out[1, 6].item() == -pi                          # [-pi, pi): +pi wraps, -pi stays
    assert abs(out[2, 6].item() - (7.0 - 2 * np.pi)) < 1e-6
    assert box[0, 6].item() == pi                                                       # the input stays
    out_np, lab_np = f(box, labels.numpy())
    assert isinstance(lab_np, np.ndarray) and lab_np.tolist() == [0, 5, 6] and torch.equal(out_np, out)
    e, el = f(torch.zeros(0, 9), torch.zeros(0, dtype=torch.long))
    assert e.shape == (0, 9) and el.shape == (0,)


def test_name_filter_drops_unknown_labels_in_order():
    names = ["car", "truck", "bus", "barrier"]
    box = torch.arange(6.0)[:, None].repeat(1, 9)
    labels = torch.tensor([2, -1, 0, 3, 1, 0])
    out, lab = A.ObjectNameFilter(names)(box, labels)
    assert lab.tolist() == [2, 0, 3, 1, 0] and out[:, 0].tolist() == [0.0, 2.0, 3.0, 4.0, 5.0]
    out, lab = A.ObjectNameFilter(["bus", "car"], class_names=names)(box, labels)
    assert lab.tolist() == [2, 0, 0] and out[:, 0].tolist() == [0.0, 2.0, 5.0]
    out, lab = A.ObjectNameFilter(names)(box, labels.numpy())
    assert isinstance(lab, np.ndarray) and lab.tolist() == [2, 0, 3, 1, 0]


# ------------------------------------------------------------------------------------------------------------ dict behaviour
def test_call_skips_missing_keys_and_takes_objects(golden):
    c = golden["a"]
    t = transform_of(c)
    # lidar2img alone: no cloud, no box
    res = t(dict(lidar2img=[m.copy() for m in c["lidar2img_in"]]), draw=draw_of(c))
    assert sorted(res) == ["lidar2img"] and np.array_equal(np.stack(res["lidar2img"]), c["lidar2img_out"])
    # plain tensors are replaced, objects keep their identity
    pts, box = magnitudes(6, 5, 1), Holder(magnitudes(2, 9, 2))
    first = box.tensor
    res = t(dict(lidar2img=[m.copy() for m in c["lidar2img_in"]], points=pts, gt_bboxes_3d=box), draw=draw_of(c))
    row = A.draw_row(draw_of(c))
    assert res["gt_bboxes_3d"] is box and torch.equal(bits(box.tensor), bits(A.bev_aug_torch(first, row, "boxes")))
    assert torch.equal(bits(res["points"]), bits(A.bev_aug_torch(pts, row, "points"))) and "radar_points" not in res
    # without a draw, one is drawn: the generator moves by two values
    np.random.seed(5)
    res = t(dict(lidar2img=[m.copy() for m in c["lidar2img_in"]], radar_points=[magnitudes(3, 7, 3)]))
    after = np.random.rand()
    np.random.seed(5)
    d = t.draw()
    assert np.random.rand() == after
    assert torch.equal(bits(res["radar_points"][0]), bits(A.bev_aug_torch(magnitudes(3, 7, 3), A.draw_row(d), "points")))


def test_prepare_bev_aug_on_cpu_tensors():
    import detector_ref as DR
    from racformer_amd import synthetic as syn
    det = DR.build(syn.SMALL)
    T, B = 2, 2
    mats = [camera((64, 96), 0.5 * v, (0.3, 0.0, 1.0)) for v in range(4)]
    metas = [dict(lidar2img=[m.copy() for m in mats], tag=b) for b in range(B)]
    radar = [[magnitudes(4 + t + b, 7, 40 + t + 2 * b) for b in range(B)] for t in range(T)]
    lidar = [magnitudes(9, 5, 50 + b) for b in range(B)]
    boxes = [magnitudes(2, 9, 60), Holder(magnitudes(3, 9, 61))]
    np.random.seed(11)
    new_metas, r2, l2, b2 = det.prepare_bev_aug(metas, radar, lidar, boxes)
    np.random.seed(11)
    t = A.RaCGlobalRotScaleTransImage()
    draws = [t.draw() for _ in range(B)]                                         # one draw per sample, in the samples' order
    assert draws[0] != draws[1]
    for b in range(B):
        row = A.draw_row(draws[b])
        assert all(np.array_equal(x, y) for x, y in zip(new_metas[b]["lidar2img"], A.view_mats(mats, draws[b])))
        assert new_metas[b]["tag"] == b and np.array_equal(metas[b]["lidar2img"][1], mats[1])           # the caller's metas stay
        assert all(torch.equal(bits(r2[t_][b]), bits(A.bev_aug_torch(radar[t_][b], row, "points"))) for t_ in range(T))
        assert torch.equal(bits(l2[b]), bits(A.bev_aug_torch(lidar[b], row, "points")))
        src = boxes[b] if isinstance(boxes[b], torch.Tensor) else boxes[b].tensor
        assert isinstance(b2[b], torch.Tensor) and torch.equal(bits(b2[b]), bits(A.bev_aug_torch(src, row, "boxes")))
    m2, r3, l3, b3 = det.prepare_bev_aug(metas, radar, draws=draws)
    assert l3 is None and b3 is None and torch.equal(r3[1][1], r2[1][1])
    with pytest.raises(ValueError, match="draws"):
        det.prepare_bev_aug(metas, radar, draws=draws[:1])
