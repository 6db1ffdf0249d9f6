"""The two image necks of ``RaCFormer.extract_img_feat`` (models/racformer.py:107-126) between the ResNet stages and the pieces
this package already has:

  ``FPN``        ``img_neck``: mmdet 2.28.2's ``FPN`` (a third-party dependency, not in the reference tree) as the f8 config builds
                 it (configs/racformer_r50_nuimg_704x256_f8.py:78-82: in [256, 512, 1024, 2048], out 256, 4 outputs).
  ``CustomFPN``  ``img_lss_neck``: the in-tree neck (models/necks/fpn.py) as configured (:89-95: in [1024, 2048], out 256,
                 ``num_outs=1, start_level=0, out_ids=[0]``); its output is the ``x`` of ``LSSViewTransformerBEVDepth_racformer``
                 and ``DepthNet``.

Both are one computation: per level a 1x1 lateral convolution with bias (no norm, no activation), coarse to fine
``laterals[i - 1] += F.interpolate(laterals[i], size=..., mode='nearest')``, then a 3x3 / pad 1 output convolution per output
level.  Two routes (``depth_net.py``'s rule):

  HIP     ``fused``, device float32 tensors and parameters, 256 output channels, every input channel count a multiple of 32, no
          gradient required: ``rac_fpn_lateral_fwd`` per level (csrc/fpn_lateral.hip: lateral convolution, bias and the top-down
          add in one launch, straight from the channel-first stage map) and the 3x3 kernel of ``FPNOutputWriter`` with a
          channel-first store (``rac_conv3x3_cf_fwd``) or, ``FPN.forward_pregrouped``, the decoder's sampling layout
          (``rac_fpn_conv_fwd``).  Split-precision f16 matrix cores at fp32-convolution accuracy; no atomics, nothing read back, launch
          geometry from the shapes alone: two runs give the same bits and a forward can be captured (inside a
          ``fused.scratch_namespace`` when plans run side by side).  Runs under ``torch.no_grad()``.
  torch   everything else -- the CPU, training, ``fused=False`` (the benchmark's baseline): ``F.conv2d`` and ``F.interpolate``.

What the f8 config does not use raises ``NotImplementedError`` in the constructors.  Backward through the HIP route and bf16 are
out of scope.  The stage maps come from the backbone of ``racformer_amd/resnet.py`` (``ResNet``), channel-first as the kernels read them."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib
from .fpn_writer import cached_pack, output_conv
from .fused import pack_conv3x3_weight

HIP_CHANNELS = 256


class _ConvModule(nn.Module):
    """mmcv's ConvModule without norm and activation: a Conv2d with bias under the key ``conv``."""

    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=k // 2)

    def forward(self, x):
        return self.conv(x)


def nearest_src(dst, in_size, out_size):
    """Source index of F.interpolate(..., size=out_size, mode='nearest') along one axis: min(int(floorf(dst * scale)), in - 1) with
    scale = (float)in / out, all in float32 (torch's nearest_neighbor_compute_source_index; what rac_fpn_lateral_fwd computes)."""
    import numpy as np
    scale = np.float32(in_size) / np.float32(out_size)
    return min(int(np.floor(np.float32(dst) * scale)), in_size - 1)


def lateral_tile_pixels(n, h, w):
    """Pixels per workgroup of rac_fpn_lateral_fwd for n images of h x w (the launcher's rule, a function of the shapes alone): 128
    where that gives every CU a workgroup, 64 below.  -> (tile, workgroups)."""
    tile = 128 if n * ((h * w + 127) // 128) >= 256 else 64
    return tile, n * ((h * w + tile - 1) // tile)


def pack_lateral_weight(weight):
    """Conv2d weight [256, Cin, 1, 1] fp32 (device) -> (f16 line image [256, Cin/32, 64] = [hi 32 | lo 32] of weight * 2^s, 2^-s)
    for rac_fpn_lateral_fwd (rac_gemm_split_pack_fwd's image); (None, None) if f16 cannot hold the weights."""
    w = weight.detach().float().reshape(weight.shape[0], -1).contiguous()
    n, k = w.shape
    amax = float(w.abs().max())
    if k % 32 != 0 or not w.is_cuda or not (amax > 0.0) or amax != amax or amax == float("inf"):
        return None, None
    s = 13 - math.frexp(amax)[1] + 1          # amax * 2^s in [2^13, 2^14)
    img = torch.empty(n, k // 32, 64, device=w.device, dtype=torch.float16)
    _lib.check(_lib.lib().rac_gemm_split_pack_fwd(_lib.ptr(w), _lib.ptr(img), n, k, float(2.0 ** s), _lib.stream_ptr()),
               "rac_gemm_split_pack_fwd")
    return img, 2.0 ** (-s)


def fpn_lateral(x, packed, bias=None, top=None):
    """x float32 device [n, Cin, H, W], ``packed`` = pack_lateral_weight of the level's weight, bias [256] or None, top [n, 256, h, w]
    (the coarser level's merged lateral, h <= H, w <= W) or None -> [n, 256, H, W] = conv1x1(x) + bias + nearest-upsampled top
    (rac_fpn_lateral_fwd)."""
    _lib.require_gpu(x, *([top] if top is not None else []), what="fpn_lateral")
    n, cin, h, w = x.shape
    img, alpha = packed
    if img is None:
        raise RuntimeError("fpn_lateral: weights cannot be held as f16 pairs (zero / non-finite weights)")
    if x.dtype != torch.float32 or tuple(img.shape) != (HIP_CHANNELS, cin // 32, 64):
        raise RuntimeError("fpn_lateral: x must be float32 [n, Cin, H, W] with Cin matching the packed weight")
    th = tw = 0
    if top is not None:
        if top.dtype != torch.float32 or top.dim() != 4 or top.shape[0] != n or top.shape[1] != HIP_CHANNELS:
            raise RuntimeError("fpn_lateral: top must be float32 [n, 256, h, w]")
        th, tw = int(top.shape[2]), int(top.shape[3])
    out = torch.empty(n, HIP_CHANNELS, h, w, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().rac_fpn_lateral_fwd(_lib.ptr(x), _lib.ptr(img), float(alpha), _lib.ptr(bias) if bias is not None else None,
                                              _lib.ptr(top) if top is not None else None, _lib.ptr(out), n, cin, h, w, th, tw,
                                              HIP_CHANNELS, _lib.stream_ptr()), "rac_fpn_lateral_fwd")
    return out


def _refuse(name, cond, what):
    if cond:
        raise NotImplementedError(f"{name}: {what} is not used by the f8 configuration and not implemented")


class _NeckBase(nn.Module):
    """Laterals, top-down path and routing shared by the two necks; subclasses own ``fpn_convs`` and the outputs."""

    def __init__(self, in_channels, out_channels, fused):
        super().__init__()
        self.in_channels, self.out_channels, self.fused = list(in_channels), out_channels, fused
        self.lateral_convs = nn.ModuleList([_ConvModule(c, out_channels, 1) for c in self.in_channels])
        self.fpn_convs = nn.ModuleList()
        self._packs = {}

    def hip_route(self, inputs):
        """True if this call runs on the kernels (the conditions of the module docstring)."""
        if not self.fused or self.out_channels != HIP_CHANNELS or any(c % 32 != 0 for c in self.in_channels):
            return False
        if not all(t.is_cuda and t.dtype == torch.float32 for t in inputs):
            return False
        if any(p.dtype != torch.float32 or not p.is_cuda for p in self.parameters()):
            return False
        if torch.is_grad_enabled() and (any(t.requires_grad for t in inputs) or any(p.requires_grad for p in self.parameters())):
            return False
        return True

    def _check(self, inputs):
        if len(inputs) != len(self.in_channels):
            raise ValueError(f"{type(self).__name__}: {len(self.in_channels)} input levels expected, got {len(inputs)}")
        for x, c in zip(inputs, self.in_channels):
            if x.dim() != 4 or x.shape[1] != c or x.shape[0] != inputs[0].shape[0]:
                raise ValueError(f"{type(self).__name__}: inputs must be [B*T*N, C_i, H_i, W_i] with C_i = {self.in_channels}")

    def laterals_torch(self, inputs):
        lat = [m(x) for m, x in zip(self.lateral_convs, inputs)]
        for i in range(len(lat) - 1, 0, -1):
            lat[i - 1] = lat[i - 1] + F.interpolate(lat[i], size=lat[i - 1].shape[2:], mode='nearest')
        return lat

    def laterals_hip(self, inputs):
        """Merged laterals, coarse to fine: one rac_fpn_lateral_fwd per level, each reading the one before as its ``top``."""
        lat, top = [None] * len(inputs), None
        for i in range(len(inputs) - 1, -1, -1):
            conv = self.lateral_convs[i].conv
            top = lat[i] = fpn_lateral(inputs[i].contiguous(), cached_pack(self._packs, ("lateral", i), conv.weight, pack_lateral_weight),
                                       conv.bias, top)
        return lat

    def _out_pack(self, j):
        return cached_pack(self._packs, ("fpn", j), self.fpn_convs[j].conv.weight, pack_conv3x3_weight)


class FPN(_NeckBase):
    """mmdet 2.28.2's ``FPN`` for the f8 configuration: one output per input level.  State-dict keys
    ``lateral_convs.{i}.conv.{weight,bias}`` and ``fpn_convs.{i}.conv.{weight,bias}`` as there (a ``FPNOutputWriter`` state dict
    loads with ``strict=False``).  ``num_cams``: images per (batch, frame), for ``forward_pregrouped``."""

    def __init__(self, in_channels, out_channels, num_outs, num_cams=6, fused=True, start_level=0, end_level=-1, add_extra_convs=False,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 upsample_cfg=dict(mode='nearest'), init_cfg=None):
        _refuse("FPN", num_outs != len(in_channels), "num_outs != len(in_channels) (extra output levels)")
        _refuse("FPN", bool(add_extra_convs) or relu_before_extra_convs, "add_extra_convs / relu_before_extra_convs")
        _refuse("FPN", start_level != 0 or end_level not in (-1, len(in_channels)), "start_level / end_level")
        _refuse("FPN", conv_cfg is not None or norm_cfg is not None or act_cfg is not None, "conv_cfg / norm_cfg / act_cfg")
        _refuse("FPN", dict(upsample_cfg) != dict(mode='nearest'), "an upsample_cfg other than dict(mode='nearest')")
        super().__init__(in_channels, out_channels, fused)
        self.num_outs, self.num_cams = num_outs, num_cams
        self.fpn_convs = nn.ModuleList([_ConvModule(out_channels, out_channels, 3) for _ in self.in_channels])

    def forward(self, inputs):
        """inputs: per level [B*T*N, C_i, H_i, W_i] -> tuple of [B*T*N, out_channels, H_i, W_i]."""
        self._check(inputs)
        if self.hip_route(inputs):
            with torch.no_grad():
                lat = self.laterals_hip(inputs)
                return tuple(output_conv(x, self._out_pack(i), self.fpn_convs[i].conv.bias, "FPN") for i, x in enumerate(lat))
        return tuple(m(x) for m, x in zip(self.fpn_convs, self.laterals_torch(inputs)))

    def forward_pregrouped(self, inputs):
        """-> per level [B*T*G, N, H_i, W_i, 64] (G = 4 groups of 64 channels, N = num_cams): the ``mlvl_feats`` of a ``pregrouped``
        decoder, written by the output convolutions themselves (rac_fpn_conv_fwd) -- no plain pyramid, no regroup pass.  HIP
        route only (``hip_route`` tells)."""
        self._check(inputs)
        if not self.hip_route(inputs):
            raise RuntimeError("FPN.forward_pregrouped: not on the HIP route (fused, device float32 tensors and parameters, 256 output "
                               "channels, input channels multiples of 32, no gradient); regroup forward()'s outputs instead")
        with torch.no_grad():
            lat = self.laterals_hip(inputs)
            return [output_conv(x, self._out_pack(i), self.fpn_convs[i].conv.bias, "FPN.forward_pregrouped", self.num_cams)
                    for i, x in enumerate(lat)]


class CustomFPN(_NeckBase):
    """The reference's ``CustomFPN`` (models/necks/fpn.py) with its constructor arguments and keys -- ``fpn_convs`` holds one entry
    per ``out_ids`` member -- for the configured shape: ``start_level=0, end_level=-1, out_ids=[0], num_outs=1``.  ``forward``
    returns the single tensor ``outs[0]`` as the reference does (:204)."""

    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, out_ids=[], add_extra_convs=False,
                 relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 upsample_cfg=dict(mode='nearest'), init_cfg=None, fused=True):
        _refuse("CustomFPN", start_level != 0 or end_level != -1, "start_level / end_level")
        _refuse("CustomFPN", list(out_ids) != [0], "out_ids other than [0]")
        _refuse("CustomFPN", num_outs != 1, "num_outs != 1 (max-pooled or extra output levels)")
        _refuse("CustomFPN", bool(add_extra_convs) or relu_before_extra_convs, "add_extra_convs / relu_before_extra_convs")
        _refuse("CustomFPN", conv_cfg is not None or norm_cfg is not None or act_cfg is not None, "conv_cfg / norm_cfg / act_cfg")
        _refuse("CustomFPN", dict(upsample_cfg) != dict(mode='nearest'), "an upsample_cfg other than dict(mode='nearest')")
        super().__init__(in_channels, out_channels, fused)
        self.num_outs, self.start_level, self.end_level, self.out_ids = num_outs, start_level, end_level, list(out_ids)
        self.fpn_convs = nn.ModuleList([_ConvModule(out_channels, out_channels, 3) for _ in self.out_ids])

    def forward(self, inputs):
        """inputs: per level [B*T*N, C_i, H_i, W_i] -> [B*T*N, out_channels, H_0, W_0], contiguous and channel-first."""
        self._check(inputs)
        if self.hip_route(inputs):
            with torch.no_grad():
                return output_conv(self.laterals_hip(inputs)[0], self._out_pack(0), self.fpn_convs[0].conv.bias, "CustomFPN")
        return self.fpn_convs[0](self.laterals_torch(inputs)[0])
