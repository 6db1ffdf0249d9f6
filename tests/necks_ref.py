"""Float64 functional restatement of the two image necks, written from the reference's lines (models/necks/fpn.py:159-180, 204:
lateral ConvModules, the coarse-to-fine ``laterals[i - 1] += F.interpolate(laterals[i], size=prev_shape, mode='nearest')``, one
output ConvModule per ``out_ids`` member, ``outs[0]`` returned) and from mmdet 2.28.2's documented ``FPN`` (the same laterals and
top-down path, one 3x3 output convolution per level, a tuple returned).  A ConvModule without norm and activation is a Conv2d with
bias (mmcv 1.6.0).  Test infrastructure: shares no code with racformer_amd/necks.py."""
import numpy as np
import torch
import torch.nn.functional as F

from racformer_amd import synthetic as syn


def nearest_index(dst, in_size, out_size):
    """Legacy 'nearest' source index along one axis (torch's nearest_neighbor_compute_source_index, float32 arithmetic)."""
    scale = np.float32(in_size) / np.float32(out_size)
    return min(int(np.floor(np.float32(dst) * scale)), in_size - 1)


def upsample_nearest(t, size):
    """F.interpolate(t, size=size, mode='nearest') by explicit indexing: [n, c, h, w] -> [n, c, H, W]."""
    H, W = size
    ih = torch.tensor([nearest_index(d, t.shape[2], H) for d in range(H)], dtype=torch.long)
    iw = torch.tensor([nearest_index(d, t.shape[3], W) for d in range(W)], dtype=torch.long)
    return t[:, :, ih][:, :, :, iw]


def lateral(x, weight, bias, top=None):
    """One level: conv1x1(x) + bias (+ upsampled top), float64."""
    out = torch.einsum("oc,nchw->nohw", weight.double().reshape(weight.shape[0], -1), x.double())
    if bias is not None:
        out = out + bias.double()[None, :, None, None]
    if top is not None:
        out = out + upsample_nearest(top, out.shape[2:])
    return out


def merged_laterals(sd, inputs):
    lat, top = [None] * len(inputs), None
    for i in range(len(inputs) - 1, -1, -1):
        top = lat[i] = lateral(inputs[i], sd[f"lateral_convs.{i}.conv.weight"], sd.get(f"lateral_convs.{i}.conv.bias"), top)
    return lat


def output_conv(sd, j, x):
    return F.conv2d(x, sd[f"fpn_convs.{j}.conv.weight"].double(), sd[f"fpn_convs.{j}.conv.bias"].double(), padding=1)


def fpn(sd, inputs):
    """mmdet FPN, num_outs == len(in_channels): tuple of float64 [n, 256, H_i, W_i]."""
    return tuple(output_conv(sd, i, x) for i, x in enumerate(merged_laterals(sd, inputs)))


def custom_fpn(sd, inputs):
    """Reference CustomFPN with out_ids=[0], num_outs=1: float64 [n, 256, H_0, W_0]."""
    return output_conv(sd, 0, merged_laterals(sd, inputs)[0])


# ---- seeded parameters and inputs shared by the fixture's generator and the tests (the fixture stores the seeds, not the weights)
def fill_state(shapes, seed):
    """shapes: {state-dict key: shape} -> {key: float32 tensor}; key number k of the sorted keys draws from seed + k, weights with
    standard deviation 1 / sqrt(fan_in), biases 0.1."""
    out = {}
    for k, key in enumerate(sorted(shapes)):
        shape = tuple(shapes[key])
        std = 0.1 if key.endswith("bias") else 1.0 / float(np.sqrt(np.prod(shape[1:])))
        out[key] = torch.from_numpy(syn.rng_normal(seed + k, shape, std))
    return out


def make_inputs(seed, images, channels, maps, relu=False):
    xs = [torch.from_numpy(syn.rng_normal(seed + i, (images, c, h, w))) for i, (c, (h, w)) in enumerate(zip(channels, maps))]
    return [x.clamp_min(0.0) for x in xs] if relu else xs


LSS = dict(channels=[64, 128], maps=[(7, 11), (4, 6)], images=2)
FPN4 = dict(channels=[32, 64, 96, 128], maps=[(16, 44), (8, 22), (4, 11), (2, 6)], images=6)
# output channels of the four-level entry kept in the fixture (all 256 of six images at four levels would be 5.8 MB): 32 channels,
# one per block of 8, at every residue modulo 8
FPN4_CHANNELS = [8 * k + (5 * k) % 8 for k in range(32)]
