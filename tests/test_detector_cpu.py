"""The detector (racformer_amd/detector.py) without a GPU: construction from the f8 ``model`` dict, the state-dict contract, what it
refuses, ``extract_feat`` / ``simple_test_offline`` on CPU tensors against the hand composition of the submodules, the streaming
bookkeeping against a dict-and-cat restatement, and ``rac_frames_gather``'s argument errors.

The decoder has no CPU route (tests/test_host_logic_cpu.py::test_no_cpu_fallback): where a test runs the head on CPU tensors, the
three HIP entry points are replaced here by the oracle's gathers and the layer runs its op-decomposed plan, as test_host_logic_cpu does."""
import copy
import ctypes

import pytest
import torch

import detector_ref as DR
import plans  # noqa: F401  (registers the reference's op decomposition: decoder_layer.fused = False)
from oracle import restate as R
from racformer_amd import RaCFormer, _lib, synthetic as syn
from racformer_amd import transformer as T
from test_host_logic_cpu import _oracle_msda, _oracle_msmv, _oracle_regroup

CFG = syn.SMALL


@pytest.fixture
def host_ops(monkeypatch):
    monkeypatch.setattr(T, "msmv_forward", _oracle_msmv)
    monkeypatch.setattr(T, "msda_forward", _oracle_msda)
    monkeypatch.setattr(T, "regroup_pyramid", _oracle_regroup)


@pytest.fixture(scope="module")
def det():
    d = DR.build(CFG)
    d.pts_bbox_head.transformer.decoder.decoder_layer.fused = False
    return d


class StubHead(torch.nn.Module):
    """A head that costs nothing, for the bookkeeping tests: one box whose coordinates are sums over the decoder's inputs."""

    def __init__(self):
        super().__init__()
        self.embed_dims = 256
        self.transformer = torch.nn.Module()
        self.transformer.decoder = torch.nn.Module()
        self.transformer.decoder.pregrouped = False
        self.seen = None

    def forward(self, mlvl_feats, lss, radar, img_metas):
        self.seen = ([f.clone() for f in mlvl_feats], lss.clone(), radar.clone(), copy.deepcopy(img_metas))
        return dict(sums=torch.stack([f.double().sum() for f in mlvl_feats] + [lss.double().sum(), radar.double().sum()]))

    def get_bboxes(self, outs, img_metas, rescale=False):
        s = outs["sums"]
        return [[torch.cat([s, s[:3]])[None].float(), s[:1].float(), torch.zeros(1, dtype=torch.long)]]


# ------------------------------------------------------------------------------------------------ construction
def test_f8_model_dict_builds_with_the_reference_keys():
    model = {k: v for k, v in DR.F8_MODEL.items() if k != "type"}
    det = RaCFormer(**model)
    assert not det.training and det.num_cams == 6
    from racformer_amd import CustomFPN, FPN, ResNet
    from racformer_amd.head import RaCFormer_head
    from racformer_amd.lss_depth import LSSViewTransformerBEVDepth_racformer
    from racformer_amd.radar_pillars import RadarPillarEncoder
    parts = {
        "img_backbone.": ResNet(**{k: v for k, v in model["img_backbone"].items() if k != "type"}),
        "img_neck.": FPN(in_channels=[256, 512, 1024, 2048], out_channels=256, num_outs=4),
        "img_lss_neck.": CustomFPN(in_channels=[1024, 2048], out_channels=256, num_outs=1, start_level=0, out_ids=[0]),
        "img_lss_view_transformer.": LSSViewTransformerBEVDepth_racformer.from_config(
            **{k: v for k, v in model["img_lss_view_transformer"].items() if k != "type"}),
        "": RadarPillarEncoder(),
        "pts_bbox_head.": RaCFormer_head(**{k: v for k, v in model["pts_bbox_head"].items() if k != "type"}),
    }
    want = {p + k: tuple(v.shape) for p, m in parts.items() for k, v in m.state_dict().items()}
    got = {k: tuple(v.shape) for k, v in det.state_dict().items()}
    assert got == want
    assert not any(k.startswith("radar_encoder.") for k in got)
    assert {k.split(".")[0] for k in got} == {"img_backbone", "img_neck", "img_lss_neck", "img_lss_view_transformer",
                                              "radar_voxel_encoder", "radar_bev_conv", "pts_bbox_head"}
    # the parts are wired as the config says
    assert det.img_backbone.input_norm == DR.NORM
    assert det.pts_bbox_head.assigner is not None and det.pts_bbox_head.loss_cls is not None     # train_cfg['pts']['assigner'] arrived
    assert det.radar_voxel_layer.max_voxels == (30000, 40000) and det.radar_middle_encoder.output_shape == (128, 128)
    assert det.radar_encoder.radar_bev_conv is det.radar_bev_conv
    # a strict round trip through another instance
    sd = {k: torch.full_like(v, 0.25) if v.is_floating_point() else v for k, v in det.state_dict().items()}
    other = RaCFormer(**model)
    other.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in other.state_dict().items())


def test_shared_lss_neck_and_built_modules():
    model = DR.small_model(CFG)
    model.update(num_lss_fpn=4)
    det = RaCFormer(**model)
    assert det.img_lss_neck is det.img_neck
    keys = set(det.state_dict())
    assert any(k.startswith("img_lss_neck.") for k in keys) and any(k.startswith("img_neck.") for k in keys)
    RaCFormer(**model).load_state_dict(det.state_dict(), strict=True)
    # already built modules are taken as they are
    model = DR.small_model(CFG)
    head = StubHead()
    model.update(pts_bbox_head=head, img_neck=det.img_neck)
    det2 = RaCFormer(**model)
    assert det2.pts_bbox_head is head and det2.img_neck is det.img_neck and det2.img_lss_neck is not det.img_neck


def test_what_it_refuses(det):
    model = DR.small_model(CFG)
    with pytest.raises(NotImplementedError, match="pre_process"):
        RaCFormer(**dict(model, pre_process=dict(type='CustomResNet')))
    with pytest.raises(NotImplementedError, match="img_backbone"):
        RaCFormer(**dict(model, img_backbone=dict(type='VoVNet')))
    with pytest.raises(NotImplementedError):
        RaCFormer(**dict(model, img_neck=dict(model["img_neck"], num_outs=5)))          # what a part refuses, the detector refuses
    a = DR.offline_args(CFG, [1, 0, 0])
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
        det(return_loss=True, **a)
    with pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
        det.forward_train(**a)
    with pytest.raises(TypeError):
        det.forward_test(img_metas=a["img_metas"][0], img=[a["img"]])
    det.train()
    try:
        with pytest.raises(NotImplementedError, match="training-mode BatchNorm"):
            det.extract_feat(**a)
    finally:
        det.eval()
    assert not det.radar_bev_conv[0].bn.training and not det.radar_encoder.training


# ------------------------------------------------------------------------------------------------ offline
def test_extract_feat_is_the_hand_composition(det):
    T, N = CFG.num_frames, CFG.num_cams
    a = DR.offline_args(CFG, [2, 1, 0])
    clouds = [p[0].clone() for p in a["radar_points"]]
    feats, bev, radar, depth = det.extract_feat(**a)
    assert [tuple(f.shape) for f in feats] == [(1, T * N, 256, h, w) for h, w in CFG.fpn_hw]
    assert tuple(bev.shape) == (1, T, 256, 16, 16) and tuple(radar.shape) == (1, T, 256, 16, 16) and tuple(depth.shape) == (N, DR.D_SMALL, 4, 11)
    assert a["img_metas"][0]["input_shape"] == (64, 176) and a["img_metas"][0]["pad_shape"][0] == (64, 176, 3)
    assert all(torch.equal(p[0], c) for p, c in zip(a["radar_points"], clouds))          # the callers' clouds stay as they are
    assert det.pts_bbox_head.transformer.decoder.pregrouped is False
    want = DR.hand_extract_feat(det, **DR.offline_args(CFG, [2, 1, 0]))[:4]
    for g, w in zip(feats + [bev, radar, depth], want[0] + list(want[1:])):
        assert g.shape == w.shape and torch.equal(g, w)
    assert float(bev.abs().max()) > 0 and float(radar.abs().max()) > 0 and not torch.equal(bev[:, 0], bev[:, 1])


def test_padding_follows_pad_multiple():
    from racformer_amd.detector import pad_multiple
    metas = [dict(ori_shape=[(30, 50, 3)] * 2)]
    x = torch.ones(2, 3, 30, 50)
    y = pad_multiple(x, metas, 32)
    assert tuple(y.shape) == (2, 3, 32, 64) and float(y[:, :, 30:].abs().sum()) == 0 and float(y[:, :, :, 50:].abs().sum()) == 0
    assert torch.equal(y[:, :, :30, :50], x) and metas[0]["img_shape"] == [(32, 64, 3)] * 2 and metas[0]["pad_shape"] == [(32, 64, 3)] * 2
    assert pad_multiple(x, metas, 10) is x


def test_simple_test_offline_is_head_and_get_bboxes(det, host_ops):
    res = det.simple_test_offline(**DR.offline_args(CFG, [2, 1, 0]))
    a = DR.offline_args(CFG, [2, 1, 0])
    feats, bev, radar, _ = det.extract_feat(**a)
    with torch.no_grad():
        outs = det.pts_bbox_head(feats, bev, radar, a["img_metas"])
        boxes, scores, labels = det.pts_bbox_head.get_bboxes(outs, a["img_metas"][0])[0]
    assert len(res) == 1 and set(res[0]) == {"pts_bbox"} and set(res[0]["pts_bbox"]) == {"boxes_3d", "scores_3d", "labels_3d"}
    got = res[0]["pts_bbox"]
    assert got["boxes_3d"].dim() == 2 and got["boxes_3d"].shape[1] == 9 and got["boxes_3d"].shape[0] > 0
    assert DR.same_result(got, dict(boxes_3d=boxes, scores_3d=scores, labels_3d=labels))
    # forward(return_loss=False) and forward_test: the reference's nesting, the same result
    a = DR.offline_args(CFG, [2, 1, 0])
    via = det(return_loss=False, img_metas=[a["img_metas"]], img=[a["img"]], radar_points=[a["radar_points"]],
              radar_depth=[a["radar_depth"]], radar_rcs=[a["radar_rcs"]])
    assert DR.same_result(via[0]["pts_bbox"], got)


# ------------------------------------------------------------------------------------------------ streaming
def test_streaming_sequence_matches_the_restatement(det, host_ops):
    det.reset_memory()
    restate = DR.Restatement(det)
    seq = DR.sequence(6, CFG.num_frames)
    assert seq[0] == [1, 0, 0] and seq[1] == [2, 1, 0] and seq[5] == [6, 5, 4]
    computed = []
    for s, fids in enumerate(seq):
        img, points, depth, rcs, metas = DR.window_inputs(CFG, fids, sample=s)
        got = det.simple_test_online(metas, img, False, points, depth, rcs)
        computed.append((det.stats["computed"], det.stats["served"]))
        want = restate(*DR.window_inputs(CFG, fids, sample=s))
        assert len(got) == 1 and DR.same_result(got[0]["pts_bbox"], want), s
        assert got[0]["pts_bbox"]["boxes_3d"].shape[0] > 0
    assert computed == [(2, 1)] + [(1, 2)] * 5 and restate.computed == [2, 1, 1, 1, 1, 1]
    assert det.stats["calls"] == 6 and det.stats["total_computed"] == 7 and det.stats["total_served"] == 11
    assert det.memory_keys() == [f"frame{f:03d}_cam0.jpg" for f in (1, 0, 2, 3, 4, 5, 6)]      # arrival order
    assert det.memory.n_slots >= 15 + CFG.num_frames
    det.reset_memory()
    assert det.memory_keys() == [] and det.stats["calls"] == 0


@pytest.fixture(scope="module")
def stub_det(det):
    model = DR.small_model(CFG)
    model.update(pts_bbox_head=StubHead(), img_backbone=det.img_backbone, img_neck=det.img_neck, img_lss_neck=det.img_lss_neck,
                 img_lss_view_transformer=det.img_lss_view_transformer, radar_voxel_encoder=det.radar_encoder)
    return RaCFormer(**model)


def test_streaming_window_is_the_cat_of_the_frames(stub_det):
    """The decoder's inputs themselves, and the cached-BEV quirk: a frame keeps the ego frame of the call that first saw it."""
    d = stub_det
    d.reset_memory()
    restate = DR.Restatement(d)
    for s, fids in enumerate(DR.sequence(3, 3)):
        img, points, depth, rcs, metas = DR.window_inputs(CFG, fids, sample=s)
        d.simple_test_online(metas, img, False, points, depth, rcs)
        feats, bev, radar, big = restate.inputs(*DR.window_inputs(CFG, fids, sample=s))
        seen = d.pts_bbox_head.seen
        assert all(g.shape == w.shape and torch.equal(g, w) for g, w in zip(seen[0] + [seen[1], seen[2]], feats + [bev, radar]))
        assert seen[3][0]["filename"] == big[0]["filename"] and len(seen[3][0]["lidar2img"]) == 9
        assert all((x == y).all() for x, y in zip(seen[3][0]["lidar2img"], big[0]["lidar2img"]))
    # frame 1 was first seen at step 0 (sample 0's ego frame); computed alone under step 2's metas its BEV map differs
    img, points, depth, rcs, metas = DR.window_inputs(CFG, [3, 2, 1], sample=2)
    fresh = d.extract_feat(img[:, 6:9], [points[2]], depth[:, 6:9], rcs[:, 6:9], DR.frame_metas(metas, 2, 3))[1]
    assert torch.equal(seen[1][:, 2], restate.cache["frame001_cam0.jpg"][1][:, 0]) and not torch.equal(seen[1][:, 2], fresh[:, 0])


def test_streaming_eviction_and_recompute(stub_det):
    d = stub_det
    d.reset_memory()
    sizes = []
    for f in range(20):
        img, points, depth, rcs, metas = DR.window_inputs(CFG, [f + 1, f], sample=0)
        d.simple_test_online(metas, img, False, points, depth, rcs)
        sizes.append(len(d.memory_keys()))
        assert d.stats["computed"] == (2 if f == 0 else 1)
        assert len(set(d.memory.slots.values())) == len(d.memory.slots)                 # no slot is held twice
    assert max(sizes) == 15 and sizes[:3] == [2, 3, 4]                                  # never 16 keys after a call
    assert d.memory_keys()[0] == "frame006_cam0.jpg" and d.memory.n_slots == 17
    assert len(d.memory.free) + len(d.memory.slots) == d.memory.n_slots
    # an evicted frame shown again is recomputed, a held one is served
    img, points, depth, rcs, metas = DR.window_inputs(CFG, [0, 20], sample=0)
    d.simple_test_online(metas, img, False, points, depth, rcs)
    assert (d.stats["computed"], d.stats["served"]) == (1, 1)
    want = DR.Restatement(d).inputs(*DR.window_inputs(CFG, [0, 20], sample=0))
    seen = d.pts_bbox_head.seen
    assert all(torch.equal(g, w) for g, w in zip(seen[0] + [seen[1], seen[2]], want[0] + [want[1], want[2]]))
    # a longer window than the ring was sized for: a new memory
    img, points, depth, rcs, metas = DR.window_inputs(CFG, [23, 22, 21], sample=0)
    d.simple_test_online(metas, img, False, points, depth, rcs)
    assert d.memory.n_slots == 18 and d.stats["computed"] == 3 and len(d.memory_keys()) == 3
    d.reset_memory()
    assert d.memory is None and d.memory_keys() == []


# ------------------------------------------------------------------------------------------------ the gather's argument errors
def test_frames_gather_argument_errors_need_no_gpu():
    lib = _lib.lib()
    one = (ctypes.c_void_p * 1)(4096)
    fb = (ctypes.c_int64 * 1)(64)
    slots = (ctypes.c_int32 * 16)(*([0] * 16))

    def call(n=1, rings=one, outs=one, frame_bytes=fb, sl=slots, T=1, n_slots=4):
        return lib.rac_frames_gather(n, rings, outs, frame_bytes, sl, T, n_slots, None), lib.rac_last_error()

    for kw, msg in ((dict(n=0), b"n_tensors"), (dict(n=9), b"n_tensors"), (dict(T=0), b"T="), (dict(T=17), b"T="),
                    (dict(rings=None), b"null pointer"), (dict(outs=None), b"null pointer"), (dict(frame_bytes=None), b"null pointer"),
                    (dict(sl=None), b"null pointer"), (dict(rings=(ctypes.c_void_p * 1)(None)), b"null pointer"),
                    (dict(outs=(ctypes.c_void_p * 1)(None)), b"null pointer"),
                    (dict(frame_bytes=(ctypes.c_int64 * 1)(24)), b"multiple of 16"), (dict(frame_bytes=(ctypes.c_int64 * 1)(0)), b"multiple of 16"),
                    (dict(sl=(ctypes.c_int32 * 1)(4)), b"outside"), (dict(sl=(ctypes.c_int32 * 1)(-1)), b"outside"),
                    (dict(sl=(ctypes.c_int32 * 2)(0, 7), T=2), b"outside"), (dict(n_slots=0), b"n_slots"),
                    (dict(rings=(ctypes.c_void_p * 1)(4100)), b"aligned")):
        rc, err = call(**kw)
        assert rc == -1 and msg in err, (kw, rc, err)
    # the wrapper's own checks come first
    from racformer_amd import fused
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        fused.frames_gather([torch.zeros(4, 8)], [torch.zeros(1, 8)], [0])
    with pytest.raises(RuntimeError, match="one out per ring"):
        fused.frames_gather([], [], [0])
