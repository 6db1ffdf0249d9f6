#!/usr/bin/env python3
"""Golden vectors of the Lift-Splat view transform: runs the REFERENCE's own LSSViewTransformer_racformer
(models/necks/view_transformer_racformer.py: create_frustum, get_lidar_coor, voxel_pooling_prepare_v2, view_transform_core)
on CPU and writes a data-only fixture next to this script.  Run in the build container only (needs the reference tree, see
ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_lss_view.py

The file is loaded with ref_loader's stubs plus the few names only this file imports: mmcv.cnn.build_conv_layer /
build_norm_layer and mmdet's BasicBlock (used by DepthNet, which is not run here: placeholders), the NECKS registry, a
``models.necks`` package path so that ``.focalloss`` resolves, and ``models.csrc.bev_pool_v2.bev_pool.bev_pool_v2``.  The
reference's pooling extension is CUDA and cannot be built here, so that last stub is a torch ``index_add_`` written below
from the operator's definition (bev_pool_cuda.cu:21-50: out[ranks_bev] += depth[ranks_depth] * feat[ranks_feat], then the
[B,C,Z,Y,X] permute of bev_pool.py:87-92); it shares no code with tests/lss_view_ref.py or racformer_amd/.

  lss_view_small.npz   keys "a:..." and "b:..." for two fixtures
      a: B=2, N=2, D=24, 4x6 feature map of a 64x96 input, C=8, a 16x16x1 grid of 6.4 m cells, ego yaws 0.07 / 0.30
      b: B=1, N=1, D=96, 2x3 feature map of a 32x48 input, C=4, a 16x16x2 grid (two z cells of 4 m: pins the z*C+c channel order)
    per fixture: grid_x/y/z/depth, input_size, downsample, lidar2img [B,N,4,4] float64, depth_digit, tran_feat, frustum,
    coor [B,N,D,H,W,3] (get_lidar_coor), ranks_bev / ranks_depth / ranks_feat / interval_starts / interval_lengths
    (voxel_pooling_prepare_v2), n_quirk (kept points with a scaled coordinate in (-1,0)), out (view_transform_core),
    state_keys.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_loader  # noqa: E402
from racformer_amd import synthetic as syn  # noqa: E402


def _bev_pool_v2(depth, feat, ranks_depth, ranks_feat, ranks_bev, bev_feat_shape, interval_starts, interval_lengths):
    c = feat.shape[-1]
    out = torch.zeros(bev_feat_shape, dtype=feat.dtype)
    out.view(-1, c).index_add_(0, ranks_bev.long(),
                               depth.reshape(-1)[ranks_depth.long()].unsqueeze(1) * feat.reshape(-1, c)[ranks_feat.long()])
    return out.permute(0, 4, 1, 2, 3).contiguous()


def load_view_transformer():
    ref_loader.load_reference()          # installs the shared stubs and the models.* namespace packages
    placeholder = lambda *a, **k: None   # noqa: E731  (DepthNet's builders: never called here)
    sys.modules["mmcv.cnn"].build_conv_layer = placeholder
    sys.modules["mmcv.cnn"].build_norm_layer = placeholder
    ref_loader._mod("mmdet.models.backbones")
    ref_loader._mod("mmdet.models.backbones.resnet", BasicBlock=type("BasicBlock", (torch.nn.Module,), {}))
    ref_loader._mod("mmdet.models.builder", NECKS=ref_loader._Registry())
    ref_loader._mod("models.csrc.bev_pool_v2").__path__ = []
    ref_loader._mod("models.csrc.bev_pool_v2.bev_pool", bev_pool_v2=_bev_pool_v2)
    pkg = types.ModuleType("models.necks")
    pkg.__path__ = [os.path.join(ref_loader.REF_ROOT, "models", "necks")]
    sys.modules["models.necks"] = pkg
    name = "models.necks.view_transformer_racformer"
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_loader.REF_ROOT, "models", "necks",
                                                                     "view_transformer_racformer.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


FIXTURES = {
    "a": dict(n_cams=2, batch=2, input_hw=(64, 96), channels=8, yaws=(0.07, 0.30), seed=3,
              grid_config=dict(x=[-51.2, 51.2, 6.4], y=[-51.2, 51.2, 6.4], z=[-5.0, 3.0, 8.0], depth=[1.0, 65.0, 24.0])),
    "b": dict(n_cams=1, batch=1, input_hw=(32, 48), channels=4, yaws=(0.07,), seed=4,
              grid_config=dict(x=[-51.2, 51.2, 6.4], y=[-51.2, 51.2, 6.4], z=[-5.0, 3.0, 4.0], depth=[1.0, 65.0, 96.0])),
}


def main():
    vt = load_view_transformer()
    out = {}
    for tag, kw in FIXTURES.items():
        inp = syn.make_lss_view_inputs(**kw)
        B, N = kw["batch"], kw["n_cams"]
        C = kw["channels"]
        m = vt.LSSViewTransformer_racformer(inp["grid_config"], inp["input_size"], downsample=inp["downsample"],
                                            in_channels=16, out_channels=C).eval()
        dd, tf = inp["depth_digit"], inp["tran_feat"]
        H, W = dd.shape[-2:]
        x = torch.zeros(B * N, 16, H, W)
        with torch.no_grad():
            coor = m.get_lidar_coor(x.view(B, N, 16, H, W), inp["img_metas"])
            rb, rd, rf, starts, lengths = m.voxel_pooling_prepare_v2(coor)
            bev, dd_out = m.view_transform_core(x, dd, tf, inp["img_metas"])
        assert dd_out is dd
        scaled = (coor - m.grid_lower_bound.to(coor)) / m.grid_interval.to(coor)
        kept = torch.zeros(coor.numel() // 3, dtype=torch.bool)
        kept[rd.long()] = True
        quirk = ((scaled > -1) & (scaled < 0)).any(-1).reshape(-1) & kept
        g = inp["grid_config"]
        fx = {"grid_x": np.asarray(g["x"], np.float64), "grid_y": np.asarray(g["y"], np.float64),
              "grid_z": np.asarray(g["z"], np.float64), "grid_depth": np.asarray(g["depth"], np.float64),
              "input_size": np.asarray(inp["input_size"], np.int64), "downsample": np.asarray(inp["downsample"], np.int64),
              "lidar2img": np.asarray([meta["lidar2img"] for meta in inp["img_metas"]], np.float64),
              "depth_digit": dd.numpy(), "tran_feat": tf.numpy(), "frustum": m.frustum.detach().numpy(),
              "coor": coor.numpy(), "ranks_bev": rb.numpy(), "ranks_depth": rd.numpy(), "ranks_feat": rf.numpy(),
              "interval_starts": starts.numpy(), "interval_lengths": lengths.numpy(),
              "n_quirk": np.asarray(int(quirk.sum()), np.int64), "out": bev.numpy(),
              "state_keys": np.asarray(sorted(m.state_dict().keys()))}
        print(tag, "points", kept.numel(), "kept", int(kept.sum()), "cells", len(starts), "fullest", int(lengths.max()),
              "quirk", int(quirk.sum()), "out", tuple(bev.shape))
        out.update({f"{tag}:{k}": v for k, v in fx.items()})
    path = os.path.join(HERE, "lss_view_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
