"""The image backbone's Bottleneck stages with given ReLU decisions, for the gradient tests: tests/resnet_ref.py's functions with
every ReLU of the named blocks replaced by a multiplication with a 0 / 1 mask.  A gradient is the gradient of the function that was
evaluated: the route under test takes its ReLU decisions from its own float32 forward, so the float64 reference is evaluated with the
same decisions (and the tests bound how many of them differ from float64's own).  Runs in the dtype of its input; shares no code with
racformer_amd."""
import torch.nn.functional as F

import resnet_ref as RR


def bottleneck(sd, p, x, stride, masks=None, own=None):
    """RR.bottleneck with ``masks`` = (m1, m2, m3) bool tensors for the three ReLUs (None: the block's own decisions); ``own``: a dict
    that receives the block's own decisions (pre-activation > 0) under ``p``."""
    a1 = RR._bn(sd, f"{p}.bn1", RR._conv(sd, f"{p}.conv1.weight", x))
    t1 = a1 * masks[0].to(a1.dtype) if masks is not None else F.relu(a1)
    a2 = RR._bn(sd, f"{p}.bn2", RR._conv(sd, f"{p}.conv2.weight", t1, stride, 1))
    t2 = a2 * masks[1].to(a2.dtype) if masks is not None else F.relu(a2)
    out = RR._bn(sd, f"{p}.bn3", RR._conv(sd, f"{p}.conv3.weight", t2))
    if f"{p}.downsample.0.weight" in sd:
        x = RR._bn(sd, f"{p}.downsample.1", RR._conv(sd, f"{p}.downsample.0.weight", x, stride))
    a3 = out + x
    if own is not None:
        own[p] = (a1.detach() > 0, a2.detach() > 0, a3.detach() > 0)
    return a3 * masks[2].to(a3.dtype) if masks is not None else F.relu(a3)


def stages(sd, x, layers, masks=None, own=None, depth=50):
    """x: the input of stage ``layers[0]`` (1-based, consecutive) -> list of those stages' outputs.  ``masks``: {block prefix:
    (m1, m2, m3)}; blocks without an entry take their own decisions."""
    outs = []
    for s in layers:
        for b in range(RR.BLOCKS[depth][s - 1]):
            p = f"layer{s}.{b}"
            x = bottleneck(sd, p, x, RR.STRIDES[s - 1] if b == 0 else 1, (masks or {}).get(p), own)
        outs.append(x)
    return outs


def resnet(sd, x, masks=None, own=None, depth=50):
    """RR.resnet with masks for the named blocks."""
    return stages(sd, RR.stem(sd, x), (1, 2, 3, 4), masks, own, depth)
