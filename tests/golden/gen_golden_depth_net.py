#!/usr/bin/env python3
"""Golden vectors of DepthNet: runs the REFERENCE's own class (models/necks/view_transformer_racformer.py:481-567, with its
ASPP / Mlp / SELayer, use_dcn=False) on CPU in float32 and writes a data-only fixture next to this script.  Run in the build
container only (needs the reference tree, see ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_depth_net.py

The class is loaded with gen_golden_lss_view.load_view_transformer(); the two placeholders that loader leaves for DepthNet's
builders are replaced here by working stand-ins written from the libraries' behaviour -- they share no code with racformer_amd/
or tests/depth_net_ref.py:
  build_norm_layer  mmcv 1.6.0: (name, layer); 'BN' -> nn.BatchNorm2d(num_features, eps=1e-5), name 'bn' + postfix
  BasicBlock        mmdet 2.28.2 resnet.BasicBlock(inplanes, planes, norm_cfg=...), stride 1, no downsample:
                    conv1 3x3 (bias=False) -> bn1 -> ReLU -> conv2 3x3 (bias=False) -> bn2 -> (+ identity) -> ReLU

  depth_net_small.npz   mid = 32, context = 16, D = 24, 2 maps; one state dict ("sd:<key>", every BatchNorm with running
                        statistics and affine parameters away from their initial values), and entry
      a: 16 x 44 maps (the f8 map: dilation 18 reaches past the image in h)
  depth_net_small.1.npz the second entry on the same state dict (a file of its own for the size limit of a committed file)
      b: 20 x 23 maps (both sizes exceed 18: all nine taps of every dilation are live somewhere)
    per entry: x, bins (int8; radar_feats = one-hot over D + 1 channels, bin D = no return), rcs_class (int8, -1..63) and
    rcs_table [32, 65] (rcs_embedding[n, :, i, j] = rcs_table[:, rcs_class[n, i, j] + 1]), mlp_input, out
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from gen_golden_lss_view import load_view_transformer  # noqa: E402

MID, CONTEXT, D, MAPS, N_RCS = 32, 16, 24, 2, 64
ENTRIES = {"a": (16, 44), "b": (20, 23)}


def build_norm_layer(cfg, num_features, postfix=''):
    cfg = dict(cfg)
    kind = cfg.pop('type')
    assert kind == 'BN', kind
    requires_grad = cfg.pop('requires_grad', True)
    cfg.setdefault('eps', 1e-5)
    layer = nn.BatchNorm2d(num_features, **cfg)
    for p in layer.parameters():
        p.requires_grad = requires_grad
    return 'bn' + str(postfix), layer


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, norm_cfg=dict(type='BN')):
        super().__init__()
        self.norm1_name, norm1 = build_norm_layer(norm_cfg, planes, postfix=1)
        self.norm2_name, norm2 = build_norm_layer(norm_cfg, planes, postfix=2)
        self.conv1 = nn.Conv2d(inplanes, planes, 3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.add_module(self.norm1_name, norm1)
        self.conv2 = nn.Conv2d(planes, planes, 3, padding=1, bias=False)
        self.add_module(self.norm2_name, norm2)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        identity = x
        out = self.conv1(x)
        out = getattr(self, self.norm1_name)(out)
        out = self.relu(out)
        out = self.conv2(out)
        out = getattr(self, self.norm2_name)(out)
        if self.downsample is not None:
            identity = self.downsample(x)
        out += identity
        return self.relu(out)


def main():
    vt = load_view_transformer()
    vt.build_norm_layer, vt.BasicBlock = build_norm_layer, BasicBlock
    torch.manual_seed(20)
    net = vt.DepthNet(MID, MID, CONTEXT, D, use_dcn=False).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, (nn.BatchNorm1d, nn.BatchNorm2d)):
                m.weight.copy_(0.6 + 0.8 * torch.rand_like(m.weight))
                m.bias.copy_(0.2 * torch.randn_like(m.bias))
                m.running_mean.copy_(0.2 * torch.randn_like(m.running_mean))
                m.running_var.copy_(0.5 + torch.rand_like(m.running_var))
    out = {"sd:" + k: v.detach().numpy() for k, v in net.state_dict().items()}
    for tag, (h, w) in ENTRIES.items():
        x = torch.randn(MAPS, MID, h, w)
        bins = torch.randint(0, D + 1, (MAPS, h, w))
        bins[torch.rand(MAPS, h, w) < 0.5] = D
        radar_feats = nn.functional.one_hot(bins, D + 1).permute(0, 3, 1, 2).float().contiguous()
        rcs_class = torch.randint(-1, N_RCS, (MAPS, h, w))
        rcs_table = 0.3 * torch.randn(32, N_RCS + 1)                  # column 0: class -1
        rcs_embedding = rcs_table[:, rcs_class + 1].permute(1, 0, 2, 3).contiguous()
        mlp_input = torch.randn(1, MAPS, 9)
        with torch.no_grad():
            y = net(x, radar_feats, rcs_embedding, mlp_input)
        assert y.shape == (MAPS, D + CONTEXT, h, w)
        # the two priors are stored as what they are gathers of (exact to rebuild; the dense tensors would not fit the size limit)
        fx = dict(x=x, bins=bins.to(torch.int8), rcs_class=rcs_class.to(torch.int8), rcs_table=rcs_table, mlp_input=mlp_input, out=y)
        for k, v in fx.items():
            out[f"{tag}:{k}"] = v.numpy()
        print(tag, "out", tuple(y.shape), "max |out|", float(y.abs().max()))
    # one file per entry keeps each under the repository's size limit (as bev_sampling_grad_small.N.npz does)
    for name, keep in (("depth_net_small.npz", ("sd:", "a:")), ("depth_net_small.1.npz", ("b:",))):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **{k: v for k, v in out.items() if k.startswith(keep)})
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
