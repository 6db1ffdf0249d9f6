#!/usr/bin/env python3
"""Golden vectors of the image necks: runs the REFERENCE's own CustomFPN (models/necks/fpn.py) on the CPU and writes a data-only
fixture next to this script.  Run in the build container only (needs the reference tree, see ref_loader.py):
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_necks.py

The file is loaded with ref_loader's stubs plus the two names only it imports: ``mmcv.cnn.ConvModule`` -- a stand-in written
below from mmcv 1.6.0's ConvModule with ``norm_cfg=None, act_cfg=None``: a Conv2d with bias under the key ``conv`` -- and mmdet's
NECKS registry.  It shares no code with tests/necks_ref.py's arithmetic or racformer_amd/.

Weights are not stored (256 x 256 x 3 x 3 fp32 does not compress): the state dict is filled from seeded normals
(tests/necks_ref.py ``fill_state``, i.e. ``racformer_amd.synthetic.rng_normal``), and the fixture stores the seeds.

  necks_small.npz
    lss:*    CustomFPN([64, 128], 256, num_outs=1, start_level=0, out_ids=[0]) on two images, maps (7, 11) and (4, 6) -- a ragged
             upsample: in0, in1, out [2, 256, 7, 11], weight_seed, state_keys
    fpn:*    the four-level neck, in [32, 64, 96, 128], maps (16, 44), (8, 22), (4, 11), (2, 6), six images.  mmdet's FPN is not
             in the reference tree; its output i equals the reference's CustomFPN(in_channels[i:], 256, num_outs=1, start_level=0,
             out_ids=[0]) on inputs[i:] with the weights lateral_convs[i:] and fpn_convs[i], which is how out0 .. out3 are made.
             The committed-file limit does not hold six images x 256 channels x four levels (5.8 MB) or their inputs (0.95 MB):
             the inputs are seeded normals too (input_seed, tests/necks_ref.py ``make_inputs``) and the outputs are kept on the 32
             channels ``channels`` (one per block of 8, every residue modulo 8): out_i [6, 32, H_i, W_i].
"""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_loader  # noqa: E402
import necks_ref as NR  # noqa: E402  (seeded parameters / inputs and the shapes only)


class ConvModule(nn.Module):
    """mmcv 1.6.0 ConvModule with norm_cfg=None and act_cfg=None: bias='auto' resolves to True without a norm, the order
    ('conv', 'norm', 'act') leaves the convolution alone."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 inplace=False):
        super().__init__()
        assert conv_cfg is None and norm_cfg is None and act_cfg is None
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=True)

    def forward(self, x):
        return self.conv(x)


def load_custom_fpn():
    ref_loader._install_stubs()
    sys.modules["mmcv.cnn"].ConvModule = ConvModule
    ref_loader._mod("mmdet.models.builder", NECKS=ref_loader._Registry())
    name = "models.necks.fpn"
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_loader.REF_ROOT, "models", "necks", "fpn.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod.CustomFPN


def shapes_of(module):
    return {k: tuple(v.shape) for k, v in module.state_dict().items()}


def main():
    CustomFPN = load_custom_fpn()
    out = {}
    # ---- the LSS neck
    seed_w, seed_x = 4100, 4200
    m = CustomFPN(NR.LSS["channels"], 256, num_outs=1, start_level=0, out_ids=[0]).eval()
    m.load_state_dict(NR.fill_state(shapes_of(m), seed_w))
    xs = NR.make_inputs(seed_x, NR.LSS["images"], NR.LSS["channels"], NR.LSS["maps"])
    with torch.no_grad():
        y = m([x.clone() for x in xs])
    out.update({"lss:in0": xs[0].numpy(), "lss:in1": xs[1].numpy(), "lss:out": y.numpy(),
                "lss:weight_seed": np.asarray(seed_w, np.int64), "lss:state_keys": np.asarray(sorted(m.state_dict()))})
    print("lss", tuple(y.shape), float(y.abs().max()))
    # ---- the four-level neck, level by level through the reference class
    seed_w, seed_x = 4300, 4400
    ch, maps, images = NR.FPN4["channels"], NR.FPN4["maps"], NR.FPN4["images"]
    full_shapes = {}
    for i, c in enumerate(ch):
        full_shapes[f"lateral_convs.{i}.conv.weight"], full_shapes[f"lateral_convs.{i}.conv.bias"] = (256, c, 1, 1), (256,)
        full_shapes[f"fpn_convs.{i}.conv.weight"], full_shapes[f"fpn_convs.{i}.conv.bias"] = (256, 256, 3, 3), (256,)
    sd = NR.fill_state(full_shapes, seed_w)
    xs = NR.make_inputs(seed_x, images, ch, maps, relu=True)
    for i in range(len(ch)):
        m = CustomFPN(ch[i:], 256, num_outs=1, start_level=0, out_ids=[0]).eval()
        part = {f"fpn_convs.0.conv.{p}": sd[f"fpn_convs.{i}.conv.{p}"] for p in ("weight", "bias")}
        for j in range(i, len(ch)):
            for p in ("weight", "bias"):
                part[f"lateral_convs.{j - i}.conv.{p}"] = sd[f"lateral_convs.{j}.conv.{p}"]
        m.load_state_dict(part)
        with torch.no_grad():
            y = m([x.clone() for x in xs[i:]])
        assert tuple(y.shape) == (images, 256) + tuple(maps[i])
        out[f"fpn:out{i}"] = y[:, NR.FPN4_CHANNELS].contiguous().numpy()
        print("fpn level", i, tuple(y.shape), float(y.abs().max()))
    out.update({"fpn:weight_seed": np.asarray(seed_w, np.int64), "fpn:input_seed": np.asarray(seed_x, np.int64),
                "fpn:channels": np.asarray(NR.FPN4_CHANNELS, np.int64), "fpn:state_keys": np.asarray(sorted(full_shapes))})
    path = os.path.join(HERE, "necks_small.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
