"""csrc/image_geom.hip on the device against ``image_geom.transform_images_numpy`` (which equals Pillow and the reference's fixture byte
for byte: tests/test_image_geom_cpu.py), BIT FOR BIT in both output kinds: the arithmetic is integer, so nothing is excused.

Every run pre-fills the output with a poison value (an element left unwritten shows), checks that the raw frames are unchanged, and
the float32 output has to hold exactly the uint8 values.  Shapes beside the fixture's are the smallest at which a path can still go
wrong: raw and output widths that are no multiple of 4 (staged rows start at every byte alignment), a raw tensor that starts at an
odd address (the first and last dwords of the tensor are assembled from bytes), output sizes that are no multiple of the 64 x 16
tile on either axis and need several tiles on both, two samples with different draws in one launch, a window wholly outside the
image, and one case at the f8 geometry (900 x 1600 -> 256 x 704 at both ends of resize_lim: the tallest and widest tiles in LDS)."""
import os

import numpy as np
import pytest
import torch

import detector_ref as DR
from racformer_amd import image_geom as G
from racformer_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
POISON_U8, POISON_F32 = 0xA5, -12345.0


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "image_geom_small.npz"))
    return {name: {k.split(":", 1)[1]: z[k] for k in z.files if k.startswith(name + ":")} for name in z["cases"]}


def draw_of(c):
    return G.IdaDraw(float(c["resize"]), tuple(int(v) for v in c["resize_dims"]), tuple(int(v) for v in c["crop"]), bool(c["flip"]),
                     float(c["rotate"]))


def noisy(shape, seed):
    """uint8 noise with saturated blocks (the bicubic lobes clip at 0 and at 255 on their edges)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, shape, dtype=np.uint8)
    n, H, W, _ = shape
    img[:, :H // 2, :W // 2] = rng.integers(0, 2, (n, H // 2, W // 2, 1)) * 255
    return img


def at_odd_address(raw):
    """The same bytes in a device tensor whose first byte is at an odd address."""
    flat = torch.empty(raw.numel() + 1, dtype=torch.uint8, device=DEV)
    view = flat[1:].view(raw.shape)
    view.copy_(raw)
    assert view.data_ptr() % 2 == 1 and view.is_contiguous()
    return view


def check(raw_np, draws, odd=False):
    """Both output kinds on the device against the numpy route, poison and read-only checks included -> the expected uint8 image."""
    m = raw_np.shape[0] // len(draws)
    want = np.concatenate([G.transform_images_numpy(raw_np[g * m:(g + 1) * m], d) for g, d in enumerate(draws)])
    raw = torch.from_numpy(raw_np).to(DEV)
    if odd:
        raw = at_odd_address(raw)
    n, fH, fW, _ = want.shape
    u8 = torch.full((n, fH, fW, 3), POISON_U8, dtype=torch.uint8, device=DEV)
    f32 = torch.full((n, 3, fH, fW), POISON_F32, dtype=torch.float32, device=DEV)
    assert G.image_geom_fwd(raw, draws, "u8_hwc", into=u8) is u8
    assert G.image_geom_fwd(raw, draws, "f32_chw", into=f32) is f32
    torch.cuda.synchronize()
    assert np.array_equal(raw.cpu().numpy(), raw_np), "the raw frames were written"
    got = u8.cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {want.size} bytes differ"
    assert np.array_equal(f32.cpu().numpy(), want.transpose(0, 3, 1, 2).astype(np.float32))
    again = G.transform_images(raw, draws, out="u8_hwc")                    # (the public route: its own tables and output)
    assert np.array_equal(again.cpu().numpy(), want)
    return want


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e"])
def test_fixture_cases_bit_for_bit(golden, name):
    c = golden[name]
    want = check(c["img"], [draw_of(c)])
    assert np.array_equal(want, c["out"])                                   # (the reference's own bytes)


def test_widths_no_multiple_of_four_and_partial_tiles():
    raw = noisy((3, 45, 83, 3), 1)                                          # rows of 249 bytes: every alignment occurs
    d = G.IdaDraw(0.9, (74, 40), (3, 5, 70, 26), True, 0.0)                 # 21 x 67: two tiles on either axis, the second 5 rows / 3 columns
    want = check(raw, [d])
    assert want.shape == (3, 21, 67, 3)
    up = G.IdaDraw(2.3, (190, 103), (20, -7, 163, 34), False, 0.0)          # up-scaled: 41 x 143, three tile rows and columns, rows above the image
    assert check(raw, [up]).shape == (3, 41, 143, 3)


def test_raw_tensor_at_an_odd_address():
    raw = noisy((2, 31, 50, 3), 2)
    d = G.IdaDraw(0.7, (35, 21), (-2, -1, 37, 22), False, 0.0)              # reads the first and the last pixel of the tensor
    want = check(raw, [d], odd=True)
    assert want[:, 1:-1, 2:-2].any() and not want[:, 0].any() and not want[:, :, :2].any()


def test_two_samples_with_different_draws_do_not_mix():
    raw = noisy((4, 45, 83, 3), 3)
    d1 = G.IdaDraw(0.5, (41, 22), (-30, -3, 70, 30), True, 0.0)             # mostly outside: the image is 41 x 22 in a 100 x 33 window
    d2 = G.IdaDraw(0.9, (74, 40), (5, 7, 105, 40), False, 0.0)              # another tap count: the tables are padded to the larger
    both = check(raw, [d1, d2])
    assert np.array_equal(both[:2], G.transform_images_numpy(raw[:2], d1)) and np.array_equal(both[2:], G.transform_images_numpy(raw[2:], d2))
    assert not np.array_equal(both[:2], G.transform_images_numpy(raw[:2], d2)[:, :, :])
    swapped = check(raw, [d2, d1])
    assert not np.array_equal(swapped, both)


def test_a_window_wholly_outside_the_image_is_zero():
    raw = noisy((2, 45, 83, 3), 4)
    for crop in [(50, -3, 150, 30), (-120, 0, -20, 33), (0, 30, 100, 63), (0, -40, 100, -7)]:
        assert not check(raw, [G.IdaDraw(0.5, (41, 22), crop, True, 0.0)]).any()


def test_f8_geometry_at_both_ends_of_resize_lim():
    raw = noisy((2, 900, 1600, 3), 5)
    lo = G.IdaDraw(0.38, (608, 342), (0, 86, 704, 342), False, 0.0)         # newW < 704: the right 96 columns are 0
    hi = G.IdaDraw(0.55, (880, 495), (131, 239, 835, 495), True, 0.0)
    want = check(raw, [lo, hi])
    assert want.shape == (2, 256, 704, 3) and not want[0, :, 608:].any() and want[0, :, :608].any()


def test_capture_and_two_replays_give_the_eager_bytes():
    raws = [noisy((4, 45, 83, 3), s) for s in (6, 7)]
    draws = [G.IdaDraw(0.9, (74, 40), (3, 5, 70, 26), True, 0.0), G.IdaDraw(0.6, (49, 27), (-4, -2, 63, 19), False, 0.0)]
    raw = torch.from_numpy(raws[0]).to(DEV)
    tables = G.device_tables(draws, (45, 83), DEV)
    u8 = torch.empty(4, 21, 67, 3, dtype=torch.uint8, device=DEV)
    f32 = torch.empty(4, 3, 21, 67, dtype=torch.float32, device=DEV)

    def launch():
        G.image_geom_fwd(raw, draws, "u8_hwc", into=u8, tables=tables)
        G.image_geom_fwd(raw, draws, "f32_chw", into=f32, tables=tables)

    launch()                                                                # (warm-up outside the capture: the module is loaded)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for data in (raws[1], raws[0]):
        raw.copy_(torch.from_numpy(data).to(DEV))
        u8.fill_(POISON_U8)
        f32.fill_(POISON_F32)
        graph.replay()
        torch.cuda.synchronize()
        eager = G.transform_images(raw, draws, out="u8_hwc").cpu().numpy()
        want = np.concatenate([G.transform_images_numpy(data[:2], draws[0]), G.transform_images_numpy(data[2:], draws[1])])
        assert np.array_equal(u8.cpu().numpy(), eager) and np.array_equal(eager, want)
        assert np.array_equal(f32.cpu().numpy(), want.transpose(0, 3, 1, 2).astype(np.float32))


def test_a_refused_shape_raises_and_launches_nothing():
    raw = torch.from_numpy(noisy((1, 180, 320, 3), 8)).to(DEV)
    d = G.IdaDraw(0.2, (64, 36), (0, 0, 64, 32), False, 0)                  # five raw positions per output position: 21 taps, 16 are held
    out = torch.full((1, 32, 64, 3), POISON_U8, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="rac_image_geom_fwd"):
        G.image_geom_fwd(raw, [d], "u8_hwc", into=out)
    torch.cuda.synchronize()
    assert bool((out == POISON_U8).all())
    with pytest.raises(NotImplementedError, match="rotate"):
        G.transform_images(raw, [d._replace(rotate=3.0)])
    with pytest.raises(ValueError, match="draws"):
        G.transform_images(raw, [d, d])


def test_prepare_raw_feeds_simple_test_offline_like_the_host_route():
    cfg, fids = syn.SMALL, [2, 1, 0]
    det = DR.build(cfg).to(DEV)
    args = DR.offline_args(cfg, fids, device=DEV)
    T, N = len(fids), cfg.num_cams
    fH, fW = cfg.image_hw
    transform = G.RandomTransformImage(dict(H=150, W=400, final_dim=(fH, fW), resize_lim=(0.45, 0.6), bot_pct_lim=(0.0, 0.1), rot_lim=(0.0, 0.0),
                                            rand_flip=True), training=True)
    raw_np = noisy((T * N, 150, 400, 3), 9)
    metas = args["img_metas"]
    np.random.seed(21)
    img, new_metas = det.prepare_raw(torch.from_numpy(raw_np).to(DEV)[None], metas, transform)
    after = np.random.rand()
    np.random.seed(21)
    draw = transform.draw()
    assert np.random.rand() == after                                        # one draw per sample
    host = dict(img=list(raw_np), lidar2img=[m.copy() for m in metas[0]["lidar2img"]])
    transform(host, draw=draw)
    host_img = torch.from_numpy(np.stack(host["img"])).permute(0, 3, 1, 2).float()[None].to(DEV)
    host_metas = [dict(metas[0], lidar2img=host["lidar2img"], ori_shape=host["ori_shape"], img_shape=host["img_shape"],
                       pad_shape=host["pad_shape"])]
    assert tuple(img.shape) == (1, T * N, 3, fH, fW) and img.dtype == torch.float32 and torch.equal(img, host_img)
    assert all(np.array_equal(a, b) and a.dtype == b.dtype for a, b in zip(new_metas[0]["lidar2img"], host_metas[0]["lidar2img"]))
    assert new_metas[0]["img_shape"] == host_metas[0]["img_shape"] == [(fH, fW, 3)] * (T * N)
    assert new_metas[0]["ori_shape"] == new_metas[0]["pad_shape"] == new_metas[0]["img_shape"] and "ori_shape" not in metas[0]
    rest = {k: v for k, v in args.items() if k not in ("img", "img_metas")}
    got = det.simple_test_offline(img_metas=new_metas, img=img, **rest)[0]["pts_bbox"]
    want = det.simple_test_offline(img_metas=host_metas, img=host_img, **rest)[0]["pts_bbox"]
    assert DR.same_result(got, want) and len(got["scores_3d"]) > 0
