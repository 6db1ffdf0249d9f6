"""Functional restatement of the image backbone by state-dict key: mmdet 2.28.2's documented ``ResNet`` with Bottleneck blocks in style
'pytorch' (stem ``conv1`` 7x7 / 2 / 3, ``bn1``, ReLU, max pool 3 / 2 / 1; per block 1x1, 3x3 with the stride, 1x1, each with an eval
BatchNorm, ``+ identity`` -- through ``downsample`` = 1x1 with the stride + BatchNorm in the first block of a stage -- and ReLU), and
the input normalisation of models/racformer.py:202-212.  It runs in the dtype of its input: float64 is the yardstick, float32 gives
E_ref.  Test infrastructure: shares no code with racformer_amd/resnet.py.

There is no golden from the reference: its tree has no ResNet-50 (models/backbones/resnet.py is ``CustomResNet``, unused with
``pre_process=None``, and imports mmdet's blocks; mmdet itself is a third-party dependency outside the tree).  Float64 torch is the
arbiter."""
import numpy as np
import torch
import torch.nn.functional as F

from racformer_amd import synthetic as syn

BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
STRIDES = (1, 2, 2, 2)
BN_FIELDS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def expected_shapes(depth, num_stages=4):
    """{state-dict key: shape} of mmdet's ResNet(depth)."""
    out = {"conv1.weight": (64, 3, 7, 7)}

    def bn(prefix, c):
        for f in BN_FIELDS:
            out[f"{prefix}.{f}"] = () if f == "num_batches_tracked" else (c,)

    bn("bn1", 64)
    inplanes = 64
    for s, blocks in enumerate(BLOCKS[depth][:num_stages]):
        planes = 64 * 2 ** s
        for b in range(blocks):
            p = f"layer{s + 1}.{b}"
            out[f"{p}.conv1.weight"] = (planes, inplanes, 1, 1)
            bn(f"{p}.bn1", planes)
            out[f"{p}.conv2.weight"] = (planes, planes, 3, 3)
            bn(f"{p}.bn2", planes)
            out[f"{p}.conv3.weight"] = (4 * planes, planes, 1, 1)
            bn(f"{p}.bn3", 4 * planes)
            if b == 0:
                out[f"{p}.downsample.0.weight"] = (4 * planes, inplanes, 1, 1)
                bn(f"{p}.downsample.1", 4 * planes)
            inplanes = 4 * planes
    return out


def expected_keys(depth):
    return sorted(expected_shapes(depth))


def fill_state(shapes, seed):
    """shapes: {state-dict key: shape} -> {key: tensor}; key number k of the sorted keys draws from seed + k.  Convolution weights
    N(0, 2 / fan_in); BatchNorm weight uniform in [0.5, 1.5], halved for every ``bn3``; BatchNorm bias and running mean N(0, 0.1^2);
    running variance uniform in [0.5, 1.5]."""
    out = {}
    for k, key in enumerate(sorted(shapes)):
        shape = tuple(shapes[key])
        field = key.rsplit(".", 1)[1]
        if field == "num_batches_tracked":
            out[key] = torch.zeros((), dtype=torch.long)
        elif len(shape) == 4:
            out[key] = torch.from_numpy(syn.rng_normal(seed + k, shape, float(np.sqrt(2.0 / np.prod(shape[1:])))))
        elif field == "weight":
            g = torch.from_numpy(syn.rng_uniform(seed + k, shape, 0.5, 1.5))
            out[key] = g * 0.5 if ".bn3." in key else g
        elif field == "running_var":
            out[key] = torch.from_numpy(syn.rng_uniform(seed + k, shape, 0.5, 1.5))
        else:
            out[key] = torch.from_numpy(syn.rng_normal(seed + k, shape, 0.1))
    return out


def input_norm(img, cfg):
    """models/racformer.py:202-212."""
    mean = torch.tensor(cfg['mean'], dtype=img.dtype)
    std = torch.tensor(cfg['std'], dtype=img.dtype)
    if cfg['to_rgb']:
        img = img[:, [2, 1, 0], :, :]
    img = img - mean.reshape(1, 3, 1, 1)
    img = img / std.reshape(1, 3, 1, 1)
    return img


def _bn(sd, prefix, x):
    t = lambda f: sd[f"{prefix}.{f}"].to(x.dtype)      # noqa: E731
    return F.batch_norm(x, t("running_mean"), t("running_var"), t("weight"), t("bias"), training=False, eps=1e-5)


def _conv(sd, key, x, stride=1, padding=0):
    return F.conv2d(x, sd[key].to(x.dtype), None, stride=stride, padding=padding)


def stem(sd, x, norm=None):
    if norm is not None:
        x = input_norm(x, norm)
    x = F.relu(_bn(sd, "bn1", _conv(sd, "conv1.weight", x, 2, 3)))
    return F.max_pool2d(x, 3, 2, 1)


def bottleneck(sd, p, x, stride):
    out = F.relu(_bn(sd, f"{p}.bn1", _conv(sd, f"{p}.conv1.weight", x)))
    out = F.relu(_bn(sd, f"{p}.bn2", _conv(sd, f"{p}.conv2.weight", out, stride, 1)))
    out = _bn(sd, f"{p}.bn3", _conv(sd, f"{p}.conv3.weight", out))
    if f"{p}.downsample.0.weight" in sd:
        x = _bn(sd, f"{p}.downsample.1", _conv(sd, f"{p}.downsample.0.weight", x, stride))
    return F.relu(out + x)


def resnet(sd, x, depth=50, norm=None):
    """-> list of the four stage outputs, in the dtype of x."""
    x = stem(sd, x, norm)
    outs = []
    for s, blocks in enumerate(BLOCKS[depth]):
        for b in range(blocks):
            x = bottleneck(sd, f"layer{s + 1}.{b}", x, STRIDES[s] if b == 0 else 1)
        outs.append(x)
    return outs


def stage_sizes(h, w):
    """(H, W) of the image -> the four stage map sizes, by the formulas of the convolution and the pool."""
    h, w = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    out = [(h, w)]
    for _ in range(3):
        h, w = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
        out.append((h, w))
    return out


NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
SEED = 5000
IMAGES = {(37, 53): 2, (32, 64): 2, (7, 9): 1, (1, 1): 1}


def make_images(hw, norm):
    """Seeded test images: plain normal, or [0, 255]-like BGR values for the normalised stem."""
    n = IMAGES[hw]
    if norm:
        return torch.from_numpy(syn.rng_uniform(SEED + 17 * hw[0] + hw[1], (n, 3) + hw, 0.0, 255.0))
    return torch.from_numpy(syn.rng_normal(SEED + 17 * hw[0] + hw[1] + 1, (n, 3) + hw))
