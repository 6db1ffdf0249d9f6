"""racformer_amd.image_geom on the host: the restatement of the reference's RandomTransformImage and of Pillow's 8-bit bicubic
resampler against the fixture the reference's own class wrote (tests/golden/gen_golden_image_geom.py), against Pillow itself where it is
installed, and negative controls that show the fixture tells the routes apart.  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from racformer_amd import _lib
from racformer_amd import image_geom as G

HERE = os.path.dirname(os.path.abspath(__file__))
PB = G.PRECISION_BITS


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "image_geom_small.npz"))
    return {name: {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(name + ":")} for name in z["cases"]}


def conf_of(c):
    return dict(H=int(c["H"]), W=int(c["W"]), final_dim=tuple(int(v) for v in c["final_dim"]), resize_lim=tuple(c["resize_lim"].tolist()),
                bot_pct_lim=tuple(c["bot_pct_lim"].tolist()), rot_lim=tuple(c["rot_lim"].tolist()), rand_flip=bool(c["rand_flip"]))


def draw_of(c):
    return G.IdaDraw(float(c["resize"]), tuple(int(v) for v in c["resize_dims"]), tuple(int(v) for v in c["crop"]), bool(c["flip"]),
                     float(c["rotate"]))


def assert_lidar2img(got, mat, before, want):
    """float32 matrix @ float64 matrix: a four-term float64 dot product whose order of summation is the BLAS's -> within 8 ulp of the
    largest product in each row."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
    prod = np.abs(mat.astype(np.float64)[None, :, :, None] * before[:, None, :, :])      # [k, row, term, col]
    tol = 8 * np.spacing(prod.max(axis=(2, 3)))                                          # [k, row]
    assert np.all(np.abs(got - want) <= tol[:, :, None]), float(np.abs(got - want).max())


# ------------------------------------------------------------------------------------------------------------ against the fixture
def test_fixture_shows_what_it_is_for(golden):
    draws = [draw_of(c) for c in golden.values()]
    assert {d.flip for d in draws} == {True, False}
    assert any(d.crop[0] > 0 for d in draws) and any(d.crop[2] > d.resize_dims[0] for d in draws) and any(d.crop[1] < 0 for d in draws)
    assert any(d.resize > 1 for d in draws) and not bool(golden["d"]["training"])
    assert any((d.resize_dims[0] == int(c["W"])) != (d.resize_dims[1] == int(c["H"])) for d, c in zip(draws, golden.values()))
    assert any(len(c["lidar2img"]) > len(c["img"]) == 6 for c in golden.values())


def test_pixels_equal_the_references_byte_for_byte(golden):
    for name, c in golden.items():
        got = G.transform_images_numpy(c["img"], draw_of(c))
        assert got.dtype == np.uint8 and np.array_equal(got, c["out"]), name
        res = G.transform_images(torch.from_numpy(c["img"]), [draw_of(c)], out="u8_hwc")          # (CPU tensors: the numpy route)
        assert np.array_equal(res.numpy(), c["out"]), name
        f32 = G.transform_images(torch.from_numpy(c["img"]), [draw_of(c)])
        assert f32.dtype == torch.float32 and np.array_equal(f32.numpy(), c["out"].transpose(0, 3, 1, 2).astype(np.float32)), name


def test_draw_makes_the_references_calls_of_the_generator(golden):
    for name, c in golden.items():
        t = G.RandomTransformImage(conf_of(c), training=bool(c["training"]))
        np.random.seed(int(c["seed"]))
        d = t.draw()
        assert np.random.rand() == float(c["next_rand"]), name
        assert d.resize == float(c["resize"]) and d.rotate == float(c["rotate"]), name
        assert d.resize_dims == tuple(c["resize_dims"]) and d.crop == tuple(c["crop"]) and d.flip == bool(c["flip"]), name
        assert all(type(v) is int for v in d.resize_dims + d.crop) and type(d.flip) is bool, name


def test_eval_draw_draws_nothing(golden):
    c = golden["d"]
    np.random.seed(5)
    before = np.random.get_state()[1].copy()
    d = G.RandomTransformImage(conf_of(c), training=False).draw()
    assert np.array_equal(np.random.get_state()[1], before) and d.rotate == 0 and d.flip is False
    assert d.resize == 0.4 and d.resize_dims == (64, 36) and d.crop == (0, 12, 64, 36)


def test_ida_mat_equals_the_references_bits(golden):
    for name, c in golden.items():
        m = G.ida_mat(draw_of(c))
        assert m.dtype == np.float32 and m.shape == (4, 4) and np.array_equal(m.view(np.uint32), c["ida_mat"].view(np.uint32)), name


def test_call_is_the_references_dict_behaviour_in_both_branches(golden):
    branches = set()
    for name, c in golden.items():
        t = G.RandomTransformImage(conf_of(c), training=bool(c["training"]))
        results = dict(img=[im.astype(np.float32) for im in c["img"]], lidar2img=[m.copy() for m in c["lidar2img"]], keep="as it is")
        np.random.seed(int(c["seed"]))
        back = t(results)
        assert back is results and results["keep"] == "as it is" and np.random.rand() == float(c["next_rand"]), name
        assert all(im.dtype == np.uint8 for im in results["img"]) and np.array_equal(np.stack(results["img"]), c["out"]), name
        assert_lidar2img(np.stack(results["lidar2img"]), c["ida_mat"], c["lidar2img"], c["lidar2img_out"])
        shapes = [tuple(s) for s in c["shape"].tolist()]
        assert results["ori_shape"] == results["img_shape"] == results["pad_shape"] == shapes, name
        branches.add(len(c["lidar2img"]) == len(c["img"]))
    assert branches == {True, False}


def test_call_raises_the_references_value_error(golden):
    c = golden["a"]
    t = G.RandomTransformImage(conf_of(c), training=False)
    first = c["img"][0]
    results = dict(img=[first] * 4, lidar2img=[c["lidar2img"][0]] * 5)
    with pytest.raises(ValueError):
        t(results)
    assert results["img"][0] is first and "img_shape" not in results       # (nothing was touched)


def test_a_given_draw_is_used(golden):
    c = golden["b"]
    results = dict(img=list(c["img"]), lidar2img=list(c["lidar2img"]))
    np.random.seed(3)
    before = np.random.get_state()[1].copy()
    G.RandomTransformImage(conf_of(c))(results, draw=draw_of(c))
    assert np.array_equal(np.random.get_state()[1], before) and np.array_equal(np.stack(results["img"]), c["out"])


def test_prepare_raw_on_cpu_tensors_is_the_dict_route(golden):
    import detector_ref as DR
    from racformer_amd import synthetic as syn
    c = golden["b"]
    det = DR.build(syn.SMALL)
    t = G.RandomTransformImage(conf_of(c))
    raw = torch.from_numpy(np.stack([c["img"], c["img"][::-1]]))                        # two samples of two frames
    metas = [dict(lidar2img=[m.copy() for m in c["lidar2img"]], tag=b) for b in range(2)]
    np.random.seed(int(c["seed"]))
    img, new = det.prepare_raw(raw, metas, t)
    np.random.seed(int(c["seed"]))
    draws = [t.draw(), t.draw()]                                                        # one draw per sample, in the samples' order
    assert draws[0] == draw_of(c) and draws[1] != draws[0]
    for b in range(2):
        host = t(dict(img=list(raw[b].numpy()), lidar2img=[m.copy() for m in c["lidar2img"]]), draw=draws[b])
        assert torch.equal(img[b], torch.from_numpy(np.stack(host["img"])).permute(0, 3, 1, 2).float())
        assert all(np.array_equal(x, y) for x, y in zip(new[b]["lidar2img"], host["lidar2img"]))
        assert new[b]["img_shape"] == new[b]["ori_shape"] == new[b]["pad_shape"] == [(48, 64, 3)] * 2 and new[b]["tag"] == b
        assert "img_shape" not in metas[b] and np.array_equal(metas[b]["lidar2img"][0], c["lidar2img"][0])      # the caller's metas stay
    assert img.dtype == torch.float32 and tuple(img.shape) == (2, 2, 3, 48, 64)
    assert np.array_equal(img[0].numpy(), c["out"].transpose(0, 3, 1, 2).astype(np.float32))
    with pytest.raises(ValueError, match="draws"):
        det.prepare_raw(raw, metas, t, draws=draws[:1])


# ------------------------------------------------------------------------------------------------------------ the coefficient tables
def test_resample_coeffs_are_pillows_tables():
    b, k = G.resample_coeffs(160, 64)                       # scale 2.5: support 5, ksize 11
    assert b.dtype == k.dtype == np.int32 and b.shape == (64, 2) and k.shape == (64, 11)
    assert b[0].tolist() == [0, 6] and b[10].tolist() == [21, 10] and b[63].tolist() == [154, 6]
    assert np.all(np.abs(k.sum(1) - (1 << PB)) <= 6)        # (each of up to 11 weights rounded to the nearest integer)
    assert np.all(k[np.arange(11)[None, :] >= b[:, 1:2]] == 0)
    bu, ku = G.resample_coeffs(60, 78)                      # up-scaling: the filter is not stretched, ksize 5
    assert ku.shape == (78, 5) and bu[:, 1].max() <= 5 and np.all(bu[:, 0] + bu[:, 1] <= 60)
    bi, ki = G.identity_coeffs(7)
    img = np.arange(7 * 3, dtype=np.uint8).reshape(7, 3) * 12
    assert np.array_equal(G.resample_pass(img, bi, ki, 0), img)


def test_resample_coeffs_refuse_an_overflowing_row(monkeypatch):
    monkeypatch.setattr(G, "PRECISION_BITS", 24)
    with pytest.raises(AssertionError, match="overflow"):
        G.resample_coeffs(160, 64)


def test_geometry_tables_fold_crop_and_flip(golden):
    c = golden["b"]                                         # 83 x 47, window (8, -4, 72, 44), flipped
    d = draw_of(c)
    tab, ks = G.geometry_tables([d], (90, 160))
    fH, fW = 48, 64
    hb, vb = tab[0, :2 * fW].reshape(fW, 2), tab[0, 2 * fW:2 * fW + 2 * fH].reshape(fH, 2)
    b, _ = G.resample_coeffs(160, 83)
    assert np.array_equal(hb, b[8:72][::-1])
    bv, _ = G.resample_coeffs(90, 47)
    assert np.all(vb[:4] == 0) and np.array_equal(vb[4:], bv[:44]) and ks == max(b[:, 1].max(), bv[:, 1].max())
    tx, ty = tab[0, 2 * (fW + fH):2 * (fW + fH) + 2], tab[0, 2 * (fW + fH) + 2:2 * (fW + fH) + 8].reshape(3, 2)
    assert tx.tolist() == [hb[:, 0].min(), (hb[:, 0] + hb[:, 1]).max()] and ty[0].tolist() == [0, bv[11].sum()]
    assert tab.shape == (1, 2 * (fW + fH) + 2 + 6 + (fW + fH) * ks)


# ------------------------------------------------------------------------------------------------------------ against Pillow itself
PIL_CASES = [(90, 160, 0.38), (90, 160, 0.55), (90, 160, 0.4731), (37, 53, 0.61), (41, 29, 0.333), (64, 64, 0.5), (19, 97, 0.77),
             (40, 60, 1.3), (23, 31, 2.17), (90, 20, 1.03), (11, 200, 0.45), (900, 1600, 0.44)]


def test_restatement_equals_pillow_on_odd_sizes():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    for i, (H, W, r) in enumerate(PIL_CASES):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        img[:H // 2, :W // 2] = rng.integers(0, 2, (H // 2, W // 2, 1)) * 255          # saturated noise: over- and undershoot
        new_w, new_h = int(W * r), int(H * r)
        d = G.IdaDraw(r, (new_w, new_h), (-3 + i, 2 - i, new_w - 5 + i, new_h + 6 - i), bool(i % 2), 0.0)
        pil = Image.fromarray(img).resize(d.resize_dims).crop(d.crop)
        if d.flip:
            pil = pil.transpose(method=Image.FLIP_LEFT_RIGHT)
        assert np.array_equal(G.transform_images_numpy(img[None], d)[0], np.array(pil.rotate(d.rotate))), (H, W, r)


# ------------------------------------------------------------------------------------------------------------ rotation
def test_rotation_raises_on_the_pixel_routes_and_keeps_the_matrix(golden):
    c = golden["b"]
    d = draw_of(c)._replace(rotate=5.4)
    with pytest.raises(NotImplementedError, match="rotate"):
        G.transform_images_numpy(c["img"], d)
    with pytest.raises(NotImplementedError, match="rotate"):
        G.transform_images(torch.from_numpy(c["img"]), [d])
    with pytest.raises(NotImplementedError, match="rotate"):
        G.geometry_tables([d], (90, 160))                   # (what the HIP route builds first)
    # img_transform's formula in float64: p' = A (F (resize p - crop[:2]) + b_flip) + (b - A b), A the rotation, F the flip
    h = d.rotate / 180 * np.pi
    A = np.array([[np.cos(h), np.sin(h)], [-np.sin(h), np.cos(h)]])
    F = np.diag([-1.0, 1.0]) if d.flip else np.eye(2)
    fH, fW = G.final_dim(d)
    b = np.array([fW, fH]) / 2
    rot = A @ F * d.resize
    tran = A @ (F @ -np.array(d.crop[:2], np.float64) + (np.array([fW, 0.0]) if d.flip else 0)) + (b - A @ b)
    want = np.eye(4)
    want[:2, :2], want[:2, 2] = rot, tran
    m = G.ida_mat(d)
    assert m.dtype == np.float32 and d.flip
    # six float32 operations at most behind an entry, each within 2^-24 of terms no larger than |crop| + fW
    tol = 6 * 2.0 ** -24 * (np.abs(d.crop).max() + fW) * 2
    assert np.abs(m - want).max() <= tol and np.abs(m[0, 1]) > 0.04


# ------------------------------------------------------------------------------------------------------------ negative controls
def raw_weights(in_size, out_size):
    """The filter's samples before Pillow normalises them."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    b, _ = G.resample_weights(in_size, out_size)
    k = np.zeros((out_size, b[:, 1].max()))
    for xx, (xmin, cnt) in enumerate(b):
        k[xx, :cnt] = G.bicubic_filter((np.arange(cnt) + xmin - (xx + 0.5) * scale + 0.5) / fs)
    return b, k


def variant(img, d, what):
    """transform_images_numpy with one thing done differently."""
    H, W = img.shape[1:3]
    new_w, new_h = d.resize_dims
    fix = lambda s: np.clip(s >> PB, 0, 255).astype(np.uint8)                      # noqa: E731
    passes = [(2, W, new_w), (1, H, new_h)]
    if what == "vertical_first":
        passes = passes[::-1]
    cur = img
    if what == "no_rounding_between":
        cur = img.astype(np.float64)
    for axis, a, b in passes:
        if a == b:
            continue
        if what == "no_rounding_between":
            bounds, w = G.resample_weights(a, b)
            m = np.zeros((b, a))
            for o, (lo, cnt) in enumerate(bounds):
                m[o, lo:lo + cnt] = w[o, :cnt]
            cur = np.moveaxis(np.tensordot(m, np.moveaxis(cur, axis, 0), 1), 0, axis)
            continue
        bounds, kk = G.resample_coeffs(a, b)
        if what == "no_half":
            cur = fix(G.resample_sums(cur, bounds, kk, axis) - (1 << (PB - 1)))
        elif what == "not_normalised":
            bounds, w = raw_weights(a, b)
            kk = np.where(w < 0, -0.5 + w * (1 << PB), 0.5 + w * (1 << PB)).astype(np.int64)
            s = sum(np.take(cur.astype(np.int64), np.minimum(bounds[:, 0] + t, a - 1), axis) * kk[:, t].reshape([-1 if i == axis else 1 for i in range(4)])
                    for t in range(kk.shape[1])) + (1 << (PB - 1))
            cur = fix(s)
        elif what == "float32":
            bounds, w = G.resample_weights(a, b)
            acc = np.zeros(cur.shape[:axis] + (b,) + cur.shape[axis + 1:], np.float32)
            for t in range(w.shape[1]):
                acc += np.take(cur.astype(np.float32), np.minimum(bounds[:, 0] + t, a - 1), axis) * w[:, t].astype(np.float32).reshape(
                    [-1 if i == axis else 1 for i in range(4)])
            cur = np.clip(np.rint(acc), 0, 255).astype(np.uint8)
        else:
            cur = G.resample_pass(cur, bounds, kk, axis)
    if what == "no_rounding_between":
        cur = np.clip(np.rint(cur), 0, 255).astype(np.uint8)
    left, upper, right, lower = d.crop
    if what == "flip_first" and d.flip:
        cur = cur[:, :, ::-1]
    if what == "clamp":
        out = cur[:, np.clip(np.arange(upper, lower), 0, new_h - 1)][:, :, np.clip(np.arange(left, right), 0, new_w - 1)]
    else:
        out = np.zeros((img.shape[0], lower - upper, right - left, 3), np.uint8)
        x0, x1, y0, y1 = max(left, 0), min(right, new_w), max(upper, 0), min(lower, new_h)
        out[:, y0 - upper:y1 - upper, x0 - left:x1 - left] = cur[:, y0:y1, x0:x1]
    if what != "flip_first" and d.flip:
        out = out[:, :, ::-1]
    return out


def test_the_variant_harness_itself_reproduces_the_fixture(golden):
    for name, c in golden.items():
        assert np.array_equal(variant(c["img"], draw_of(c), "none"), c["out"]), name


@pytest.mark.parametrize("what", ["no_half", "vertical_first", "no_rounding_between", "not_normalised", "float32", "flip_first", "clamp"])
def test_negative_controls_fail_against_the_fixture(golden, what):
    differing = [name for name, c in golden.items() if not np.array_equal(variant(c["img"], draw_of(c), what), c["out"])]
    assert differing, f"the fixture cannot tell the restatement from the '{what}' variant"


# ------------------------------------------------------------------------------------------------------------ the entry point's refusals
def call_entry(tab, ks, raw_hw, out_hw, n=1, group=1):
    host = np.ascontiguousarray(tab, np.int32)
    fake = ctypes.c_void_p(64)                  # (never dereferenced: every call below is refused before any HIP call)
    rc = _lib.lib().rac_image_geom_fwd(fake, fake, host.ctypes.data_as(ctypes.c_void_p), fake, n, group, raw_hw[0], raw_hw[1], out_hw[0],
                                       out_hw[1], ks, G.OUT_F32_CHW, None)
    return rc, _lib.lib().rac_last_error().decode()


def test_entry_point_refuses_before_any_launch():
    d = G.IdaDraw(0.2, (64, 36), (0, 0, 64, 32), False, 0)                  # 320 x 180 -> 64 x 36: five raw positions per output position
    tab, ks = G.geometry_tables([d], (180, 320))
    rc, msg = call_entry(tab, ks, (180, 320), (32, 64))
    assert rc == -2 and "rac_image_geom_fwd" in msg and "too strong" in msg
    d = G.IdaDraw(0.4, (64, 36), (0, 12, 64, 36), False, 0)
    tab, ks = G.geometry_tables([d], (90, 160))
    rc, msg = call_entry(tab, ks, (90, 159), (24, 64))                      # a raw image narrower than the tables were made for
    assert rc == -1 and "rac_image_geom_fwd" in msg and "column" in msg
    bad = tab.copy()
    bad[0, 2 * 64 + 1] = ks + 1                                             # row 0: more taps than the table holds
    rc, msg = call_entry(bad, ks, (90, 160), (24, 64))
    assert rc == -1 and "taps" in msg
    rc, msg = call_entry(tab, ks, (90, 160), (24, 64), n=3, group=2)
    assert rc == -1 and "groups" in msg
    assert _lib.lib().rac_image_geom_fwd(None, None, None, None, 0, 1, 90, 160, 24, 64, ks, G.OUT_U8_HWC, None) == 0      # no images: nothing to do
