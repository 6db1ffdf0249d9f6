"""The detector's input side on the device at synthetic.SMALL: with ``radar_depth=None, radar_rcs=None`` the maps come from
``rac_point_maps_radar_fwd`` (racformer_amd/point_maps.py) and every entry point -- ``extract_feat``, ``simple_test_offline``, a cold
and two steady ``simple_test_online`` steps (the second one a captured replay) -- gives bit for bit what the same call gives with
``point_maps.radar_maps``' result passed in; ``forward_train(gt_depth=None, points=...)`` gives the ``loss_depth`` bits of the same
call with ``point_maps.lidar_depth_map``'s result passed in."""
import pytest
import torch

import detector_ref as DR
import detector_train_ref as TR
from racformer_amd import point_maps as PM, synthetic as syn
from test_detector_maps_cpu import args, built_maps, flat, same

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CFG = syn.SMALL
WINDOW = [2, 1, 0]


@pytest.fixture(scope="module")
def det():
    return DR.build(CFG).to(DEV)


def test_extract_feat_and_offline(det):
    e = args(True, device=DEV)
    assert e["radar_depth"].is_cuda
    want = det.extract_feat(**e)
    got = det.extract_feat(**args(False, device=DEV))
    assert same(flat(got), flat(want))
    on_cpu = args(True)                              # the device's maps are the restatement's, bit for bit
    assert torch.equal(e["radar_depth"].cpu(), on_cpu["radar_depth"]) and torch.equal(e["radar_rcs"].cpu(), on_cpu["radar_rcs"])
    res = det.simple_test_offline(**args(False, device=DEV))[0]["pts_bbox"]
    assert res["boxes_3d"].shape[0] > 0 and DR.same_result(res, det.simple_test_offline(**args(True, device=DEV))[0]["pts_bbox"])


def test_streaming_cold_and_steady(det):
    results = {}
    for explicit in (True, False):
        det.reset_memory()
        results[explicit] = []
        for s, fids in enumerate(DR.sequence(3, CFG.num_frames)):
            img, points, _, _, metas = DR.window_inputs(CFG, fids, sample=s, device=DEV)
            maps = built_maps(points, metas, CFG.image_hw, DR.GRID_SMALL, CFG.num_cams, DEV) if explicit else (None, None)
            res = det.simple_test_online(metas, img, False, points, *maps)
            results[explicit].append((res[0]["pts_bbox"], det.stats["computed"], det._plan is not None))
    det.reset_memory()
    for a, b in zip(results[True], results[False]):
        assert a[0]["boxes_3d"].shape[0] > 0 and DR.same_result(a[0], b[0]) and a[1:] == b[1:]
    assert [r[1:] for r in results[False]] == [(2, False), (1, True), (1, True)]


def test_forward_train_makes_gt_depth_from_the_lidar_clouds():
    det = DR.build(CFG).to(DEV)
    det.fused_grad = True
    det.train()
    state = {k: v.clone() for k, v in det.state_dict().items()}
    H, W = CFG.image_hw

    def step(explicit):
        det.load_state_dict(state)
        a = TR.train_args(CFG, (3, 2), device=DEV)
        # lidar clouds: the samples' radar clouds of two frames, spread out (some points leave the views or the depth range)
        clouds = [torch.cat([a["radar_points"][0][b][:, :5] * 3.0, a["radar_points"][1][b][:, :5] * 2.0]) for b in range(2)]
        a["radar_depth"] = a["radar_rcs"] = None
        if explicit:
            pts, off = PM.pack_clouds(clouds)
            gt = PM.lidar_depth_map(pts, off, PM.meta_view_table(a["img_metas"], CFG.num_cams, frames=1), (H, W), DR.GRID_SMALL,
                                    pad_hw=a["gt_depth"].shape[-2:])
            assert gt.is_cuda and gt.count_nonzero() > 0
            a["gt_depth"] = gt.view(2, CFG.num_cams, *gt.shape[-2:])
        else:
            a["gt_depth"], a["points"] = None, clouds
        TR.seed_all(5)
        return {k: v.detach().clone() for k, v in det.forward_train(**a).items()}

    want, got = step(True), step(False)
    assert set(got) == set(want) and float(want["loss_depth"]) > 0
    assert torch.equal(got["loss_depth"], want["loss_depth"])
    assert all(torch.equal(got[k], want[k]) for k in want)
