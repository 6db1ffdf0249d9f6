#!/usr/bin/env python3
"""Golden vectors of the LSS depth branch: runs the REFERENCE's own LSSViewTransformerBEVDepth_racformer
(models/necks/view_transformer_racformer.py:572-699: get_downsampled_depth, get_downsampled_rcs, the prior tensors forward hands
to DepthNet, get_depth_loss with models/necks/focalloss.py) on CPU, float32, and writes a data-only fixture next to this script.
Run in the build container only (needs the reference tree, see ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_lss_depth.py

Loaded with the import stubs of gen_golden_lss_view.py.  DepthNet (mmcv's DCN, mmdet's BasicBlock) cannot be built here and is not
what this fixture pins: the module's ``DepthNet`` name is bound to a recorder that keeps the two prior tensors ``forward`` passes
to it and returns its input; ``view_transform`` is bound to a pass-through for the same call.

  lss_depth_small.npz   keys "a:..." and "b:..."
      a: B*N = 2 (B=1, N=2), 32 x 48 maps, ds = 8,  D = 24, depth [1, 65], rcs [-64, 64, 64]
      b: B*N = 1,            64 x 96 maps, ds = 16, D = 96
    per fixture: grid_depth, grid_rcs, downsample, radar_depth / radar_rcs / lidar_depth [B,N,H,W], rad_inds int64 and
    radar_pooled (get_downsampled_depth of the radar map), rcs_one_hot (get_downsampled_rcs), rad_dep_grids and rcs_embedding
    (forward's arguments to DepthNet), rcs_weight / rcs_bias, depth_preds [B*N,D,h,w], label_inds / label_pooled
    (get_downsampled_depth of the lidar map), loss (get_depth_loss), grad_preds (autograd), grad_rcs_weight / grad_rcs_bias
    (autograd of sum(rcs_embedding * prior_gout)), prior_gout, state_keys.
  and "edges:depths" / "edges:inds": get_downsampled_depth (ds = 1, depth [1, 65, 96]) on the constructed bin edges
  d_k = lo + bin k (k + 1) / 2, k = 0..97, their float32 neighbours and 0, 0.5, 1e5, inf, nan, -3 (lss_depth_ref.edge_depths).
Inputs: synthetic.make_lss_depth_inputs with every_block_has_rcs, so that the reference's F.one_hot does not raise.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from gen_golden_lss_view import load_view_transformer  # noqa: E402
from racformer_amd import synthetic as syn  # noqa: E402

sys.path.insert(0, os.path.dirname(HERE))
import lss_depth_ref  # noqa: E402  (edge_depths only: the list of inputs, no arithmetic of the restatement)

FIXTURES = {
    "a": dict(batch=1, n_cams=2, input_hw=(32, 48), downsample=8, depth=[1.0, 65.0, 24.0], seed=1, radar_density=0.05),
    "b": dict(batch=1, n_cams=1, input_hw=(64, 96), downsample=16, depth=[1.0, 65.0, 96.0], seed=2, radar_density=0.02),
}
RCS = [-64, 64, 64]


class Recorder(torch.nn.Module):
    def __init__(self, *a, **k):
        super().__init__()
        self.seen = None

    def forward(self, x, radar_feats, rcs_embedding, mlp_input):
        self.seen = (radar_feats, rcs_embedding)
        return x


def main():
    vt = load_view_transformer()
    vt.DepthNet = Recorder
    out = {}
    for tag, kw in FIXTURES.items():
        B, N, ds = kw["batch"], kw["n_cams"], kw["downsample"]
        H, W = kw["input_hw"]
        D = int(kw["depth"][2])
        grid = dict(x=[-51.2, 51.2, 6.4], y=[-51.2, 51.2, 6.4], z=[-5.0, 3.0, 8.0], depth=kw["depth"], rcs=RCS)
        torch.manual_seed(kw["seed"])
        m = vt.LSSViewTransformerBEVDepth_racformer(grid_config=grid, input_size=kw["input_hw"], downsample=ds, in_channels=16,
                                                    out_channels=8, loss_depth_weight=2.0)
        m.view_transform = lambda x, depth_digit, tran_feat, img_metas: (tran_feat, depth_digit)
        inp = syn.make_lss_depth_inputs(n_maps=B * N, input_hw=kw["input_hw"], downsample=ds, seed=kw["seed"],
                                        radar_density=kw["radar_density"])
        radar_depth, radar_rcs, lidar = (inp[k].view(B, N, H, W) for k in ("radar_depth", "radar_rcs", "lidar_depth"))
        h, w = H // ds, W // ds
        rad_inds, radar_pooled = m.get_downsampled_depth(radar_depth, ds)
        one_hot = m.get_downsampled_rcs(radar_rcs, ds)
        m(torch.zeros(B, N, D + 8, h, w), radar_depth, radar_rcs, None, None)
        rad_dep_grids, rcs_embedding = m.depth_net.seen
        gout = torch.from_numpy(syn.rng_normal(kw["seed"] * 1000 + 83, tuple(rcs_embedding.shape)))
        gw, gb = torch.autograd.grad((rcs_embedding * gout).sum(), (m.rcs_embedding.weight, m.rcs_embedding.bias))
        preds = torch.from_numpy(syn.rng_normal(kw["seed"] * 1000 + 82, (B * N, D, h, w), scale=2.0)).requires_grad_(True)
        label_inds, label_pooled = m.get_downsampled_depth(lidar, ds)
        loss = m.get_depth_loss(lidar, preds)
        (gp,) = torch.autograd.grad(loss, preds)
        fx = {"grid_depth": np.asarray(kw["depth"], np.float64), "grid_rcs": np.asarray(RCS, np.float64),
              "downsample": np.asarray(ds, np.int64), "loss_depth_weight": np.asarray(2.0, np.float64),
              "radar_depth": radar_depth.numpy(), "radar_rcs": radar_rcs.numpy(), "lidar_depth": lidar.numpy(),
              "rad_inds": rad_inds.numpy(), "radar_pooled": radar_pooled.numpy(), "rcs_one_hot": one_hot.numpy().astype(np.uint8),
              "rad_dep_grids": rad_dep_grids.detach().contiguous().numpy().astype(np.uint8),
              "rcs_embedding": rcs_embedding.detach().numpy(), "rcs_weight": m.rcs_embedding.weight.detach().numpy(),
              "rcs_bias": m.rcs_embedding.bias.detach().numpy(), "depth_preds": preds.detach().numpy(),
              "label_inds": label_inds.numpy(), "label_pooled": label_pooled.numpy(), "loss": loss.detach().numpy(),
              "grad_preds": gp.numpy(), "prior_gout": gout.numpy(), "grad_rcs_weight": gw.numpy(), "grad_rcs_bias": gb.numpy(),
              "state_keys": np.asarray(sorted(m.state_dict().keys()))}
        print(tag, "radar foreground", int((rad_inds < D).sum()), "of", rad_inds.numel(), "lidar foreground",
              int((label_inds < D).sum()), "rcs classes", int(one_hot.sum()), "loss", float(loss.detach()))
        out.update({f"{tag}:{k}": v for k, v in fx.items()})
    edges = lss_depth_ref.edge_depths(FIXTURES["b"]["depth"])
    inds, _ = m.get_downsampled_depth(torch.from_numpy(edges).view(1, 1, 1, -1), 1)        # (m: fixture b's module, D = 96)
    out["edges:depths"], out["edges:inds"] = edges, inds.view(-1).numpy()
    path = os.path.join(HERE, "lss_depth_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
