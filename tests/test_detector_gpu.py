"""The detector on the device (racformer_amd/detector.py) at synthetic.SMALL: extract_feat and simple_test_offline against the hand
composition of the device submodules (bitwise), the streaming route -- ring, rac_frames_gather, CapturedStep.replay -- against the
dict-and-cat restatement (bitwise), the four outputs of extract_feat against the same detector on CPU float64 under the rules of
the stages' own tests, and streaming against offline on a static scene.

Accuracy is inherited from the per-stage tests; what is new here is the chain.  The rules: the pyramid under ``within_rule`` of
tests/test_resnet_gpu.py with the stage count of its ``test_chain_into_the_necks``; the BEV map and the depth logits under
``RATIO * E_ref`` (+ one ulp at the tensor's scale for the BEV map) of tests/test_depth_net_gpu.py::test_4; the radar stack under the
derived bound of tests/test_radar_pillars_gpu.py::test_5.  ``E_ref`` is the CPU float32 run's own error against float64.  A chained
BEV map / depth tensor that exceeds its rule is judged teacher-forced (the CPU modules fed the device's own ``img_lss_feats``); both
figures go to the file named by RAC_DETECTOR_ERRORS (profiles/detector_small.json).  Measured on an MI355X: the chained depth passes
(7.3e-4 against 2.5e-3 allowed); the chained BEV map misses its rule (1.97e-2 against 1.46e-2 allowed, at a scale of 3654) and passes
teacher-forced (5.1e-3 against 6.9e-2 allowed)."""
import json
import os

import pytest
import torch

import detector_ref as DR
import radar_pillars_ref as RPR
from racformer_amd import synthetic as syn
from racformer_amd.lss_view import RankTables
from test_depth_net_gpu import RATIO
from test_radar_pillars_gpu import CONV_RTOL, IMAGE_RES, in_range_absmax, pfn_bound
from test_resnet_gpu import STAGES, within_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = syn.SMALL
WINDOW = [2, 1, 0]
FIGURES = {}


@pytest.fixture(scope="module", autouse=True)
def _figures():
    yield
    path = os.environ.get("RAC_DETECTOR_ERRORS")
    if path:
        with open(path, "w") as f:
            json.dump(FIGURES, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def det():
    return DR.build(CFG).to(DEV)


def dev_args(fids, sample=0):
    return DR.offline_args(CFG, fids, sample, device=DEV)


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ offline, bitwise
def test_extract_feat_is_the_hand_composition(det):
    T, N = CFG.num_frames, CFG.num_cams
    feats, bev, radar, depth = det.extract_feat(**dev_args(WINDOW))
    assert det.pts_bbox_head.transformer.decoder.pregrouped is True          # the neck's HIP route holds: the sampling layout
    assert [tuple(f.shape) for f in feats] == [(T * 4, N, h, w, 64) for h, w in CFG.fpn_hw]
    assert tuple(bev.shape) == (1, T, 256, 16, 16) and tuple(radar.shape) == (1, T, 256, 16, 16) and tuple(depth.shape) == (N, DR.D_SMALL, 4, 11)
    want = DR.hand_extract_feat(det, **dev_args(WINDOW))
    assert all(bits_equal(g, w) for g, w in zip(feats + [bev, radar, depth], want[0] + list(want[1:4])))
    again = det.extract_feat(**dev_args(WINDOW))
    assert all(bits_equal(g, w) for g, w in zip(feats + [bev, radar, depth], again[0] + list(again[1:])))
    # pregrouped off: the reference's layout, the same numbers
    det.pregrouped = False
    try:
        plain = det.extract_feat(**dev_args(WINDOW))
        assert det.pts_bbox_head.transformer.decoder.pregrouped is False
        assert [tuple(f.shape) for f in plain[0]] == [(1, T * N, 256, h, w) for h, w in CFG.fpn_hw]
        assert all(bits_equal(DR.ungroup(g, T), p) for g, p in zip(feats, plain[0]))
        assert bits_equal(bev, plain[1]) and bits_equal(radar, plain[2])
    finally:
        det.pregrouped = True


def test_simple_test_offline_is_head_and_get_bboxes(det):
    res = det.simple_test_offline(**dev_args(WINDOW))
    a = dev_args(WINDOW)
    feats, bev, radar, _ = det.extract_feat(**a)
    with torch.no_grad():
        outs = det.pts_bbox_head(feats, bev, radar, a["img_metas"])
        boxes, scores, labels = det.pts_bbox_head.get_bboxes(outs, a["img_metas"][0])[0]
    got = res[0]["pts_bbox"]
    assert got["boxes_3d"].shape[1] == 9 and got["boxes_3d"].shape[0] > 0 and not got["boxes_3d"].is_cuda
    assert DR.same_result(got, dict(boxes_3d=boxes.cpu(), scores_3d=scores.cpu(), labels_3d=labels.cpu()))
    assert DR.same_result(det.simple_test_offline(**dev_args(WINDOW))[0]["pts_bbox"], got)          # two runs, the same bits


# ------------------------------------------------------------------------------------------------ streaming, bitwise
def test_streaming_sequence_matches_the_restatement(det):
    det.reset_memory()
    restate = DR.Restatement(det)
    computed, replayed = [], []
    for s, fids in enumerate(DR.sequence(6, CFG.num_frames)):
        img, points, depth, rcs, metas = DR.window_inputs(CFG, fids, sample=s, device=DEV)
        got = det.simple_test_online(metas, img, False, points, depth, rcs)
        computed.append(det.stats["computed"])
        replayed.append(det._plan is not None)
        want = restate(*DR.window_inputs(CFG, fids, sample=s, device=DEV))              # eager: the head on torch.cat of the frames
        assert DR.same_result(got[0]["pts_bbox"], want), s
        assert got[0]["pts_bbox"]["boxes_3d"].shape[0] > 0
    assert computed == [2, 1, 1, 1, 1, 1] and restate.computed == computed
    assert replayed == [False] + [True] * 5                                              # after the warm-up: CapturedStep.replay
    assert det.memory.pregrouped and all(r.is_cuda and r.shape[0] == 15 + CFG.num_frames for r in det.memory.rings)
    window = [w.data_ptr() for w in det._window]
    assert window == [t.data_ptr() for t in det._plan.inputs[0]] + [det._plan.inputs[1].data_ptr(), det._plan.inputs[2].data_ptr()]
    det.reset_memory()
    assert det.memory is None and det._plan is None


# ------------------------------------------------------------------------------------------------ accuracy of the chain
@pytest.fixture(scope="module")
def chain(det):
    """The device's extract_feat on WINDOW in the reference's layout, and the CPU float64 / float32 runs of the same detector (hand
    composition; the CPU view transformers splat on the device's cell table, as tests/test_depth_net_gpu.py::test_4 does)."""
    T = CFG.num_frames
    feats, bev, radar, depth = det.extract_feat(**dev_args(WINDOW))
    lss = DR.hand_extract_feat(det, **dev_args(WINDOW), radar=False)[4]
    a = dev_args(WINDOW)
    frame0 = [dict(lidar2img=a["img_metas"][0]["lidar2img"][:CFG.num_cams])]
    cells = det.img_lss_view_transformer._rank_tables(depth.contiguous(), frame0).cells.cpu().long()     # one rig for every frame
    got = dict(pyramid=[DR.ungroup(f, T).cpu() for f in feats], bev=bev.cpu(), radar=radar.cpu(), depth=depth.cpu(), lss=lss.cpu())
    ref, forced = {}, {}
    for dtype in (torch.float64, torch.float32):
        cpu = DR.build(CFG).to(dtype)
        vt = cpu.img_lss_view_transformer
        vt.accelerate, vt.ranks, vt.initial_flag = True, RankTables(cells, None, None, None, None, None, None), False
        args = DR.offline_args(CFG, WINDOW, dtype=dtype)
        out = DR.hand_extract_feat(cpu, **args, dtype=dtype, radar=False)
        ref[dtype] = dict(pyramid=out[0], bev=out[1], depth=out[3])
        out = DR.hand_extract_feat(cpu, **DR.offline_args(CFG, WINDOW, dtype=dtype), dtype=dtype, radar=False, lss_feats=got["lss"].to(dtype))
        forced[dtype] = dict(bev=out[1], depth=out[3])
    return got, ref, forced


def test_pyramid_against_float64(chain):
    got, ref, _ = chain
    for lvl in range(4):
        within_rule(f"detector pyramid level {lvl}", got["pyramid"][lvl], ref[torch.float64]["pyramid"][lvl], ref[torch.float32]["pyramid"][lvl],
                    stages=STAGES[3] + 2, group="detector")


@pytest.mark.parametrize("name", ["bev", "depth"])
def test_bev_and_depth_against_float64(chain, name):
    got, ref, forced = chain

    def figures(r):
        r64, r32 = r[torch.float64][name], r[torch.float32][name]
        e_ref = float((r32.double() - r64).abs().max())
        tol = RATIO * e_ref + (2.0 ** -23 * float(r64.abs().max()) if name == "bev" else 0.0)
        return dict(e_ref=e_ref, err=float((got[name].double() - r64).abs().max()), allowed=tol, scale=float(r64.abs().max()))

    chained, tf = figures(ref), figures(forced)
    FIGURES[name] = dict(chained=chained, teacher_forced=tf)
    print(f"{name}: chained {chained}, teacher-forced {tf}")
    assert float(got[name].abs().sum()) > 0
    if chained["err"] > chained["allowed"]:
        assert tf["err"] <= tf["allowed"], (name, chained, tf)


def test_radar_stack_against_float64(chain):
    got = chain[0]["radar"]
    sd = DR.part_state_dicts(CFG)[""]
    cfg = dict(DR.RADAR_SMALL)
    clouds = [DR.frame_inputs(CFG, f)[3] for f in WINDOW]
    frames = [[c] for c in clouds]
    want, stages = RPR.forward(sd, cfg, frames, torch.float64)
    st = RPR.Stages(sd, torch.float64, **cfg)
    e_ref = 0.0
    for fr in frames:
        v, c, n = RPR.voxelize_batch(fr, zero_z=True, **cfg)
        e_ref = max(e_ref, RPR.canvas_e_ref(sd, cfg, v, c, n, 1)[1])
    tol = [RATIO * e_ref + IMAGE_RES * pfn_bound(sd, cfg, in_range_absmax(clouds, cfg))]
    tol += [CONV_RTOL * max(float(s[i + 1].abs().max()) for s in stages) for i in range(3)]
    gain = [st.folded_conv_l1(i) for i in range(3)]
    bound = tol[0] * gain[0] * gain[1] * gain[2] + tol[1] * gain[1] * gain[2] + tol[2] * gain[2] + tol[3]
    err = float((got.double() - want).abs().max())
    FIGURES["radar"] = dict(err=err, allowed=bound)
    print(f"radar stack: error {err:.3g}, derived bound {bound:.3g}")
    assert tuple(got.shape) == tuple(want.shape) and err <= bound


def test_streaming_against_offline_on_a_static_scene(det, chain):
    """The same metas every step: the decoder's inputs of the streaming route (frames computed one at a time) may differ from the
    offline route's (all frames in one batch) by no more than the offline route's own error against float64."""
    got, ref, _ = chain
    T = CFG.num_frames
    det.reset_memory()
    for fids in DR.sequence(2, T):
        img, points, depth, rcs, metas = DR.window_inputs(CFG, fids, sample=0, device=DEV)
        det.simple_test_online(metas, img, False, points, depth, rcs)
    assert DR.sequence(2, T)[-1] == WINDOW
    win = [w.clone() for w in det._window]
    det.reset_memory()
    stream = dict(pyramid=[DR.ungroup(w, T).cpu() for w in win[:4]], bev=win[4].cpu(), radar=win[5].cpu())
    sd = DR.part_state_dicts(CFG)[""]
    radar64 = RPR.forward(sd, dict(DR.RADAR_SMALL), [[DR.frame_inputs(CFG, f)[3]] for f in WINDOW], torch.float64)[0]
    pairs = [(f"pyramid{l}", stream["pyramid"][l], got["pyramid"][l], ref[torch.float64]["pyramid"][l]) for l in range(4)]
    pairs += [("bev", stream["bev"], got["bev"], ref[torch.float64]["bev"]), ("radar", stream["radar"], got["radar"], radar64)]
    bad = []
    for name, s, o, r64 in pairs:
        diff, own = float((s.double() - o.double()).abs().max()), float((o.double() - r64).abs().max())
        FIGURES[f"static:{name}"] = dict(streaming_vs_offline=diff, offline_vs_float64=own)
        print(f"static scene {name}: streaming - offline {diff:.3g}, offline - float64 {own:.3g}")
        if diff > own:
            bad.append((name, diff, own))
    assert not bad, bad
