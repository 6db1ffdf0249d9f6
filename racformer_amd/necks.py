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
  HIP, training   the same conditions with autograd recording and the class attribute ``fused_grad`` set (opt-in, default False;
          ``hip_grad_route``): ``forward`` runs the same launches through one ``torch.autograd.Function`` (``_NeckCore``) and returns
          the same bits; the backward walks the levels fine to coarse -- the 3x3 data and weight gradients on the kernels the
          temporal-fusion convolution uses under autograd (``rac_conv3x3_cf_fwd`` with ``fused.pack_conv3x3_dgrad_weight``'s weights,
          ``rac_conv3x3_wgrad``), the top-down add backwards as a gather over each coarse pixel's children (``rac_fpn_merge_bwd``,
          ``nearest_children``), the lateral weight / bias gradient (``rac_fpn_lateral_wgrad``) and the lateral data gradient
          (``rac_fpn_lateral_dgrad``, the forward's kernel on W^T) -- skipping whatever ``requires_grad`` does not ask for (with
          ``frozen_stages=1`` the stage-0 map needs no gradient: the largest data gradient is never launched).  Fixed summation
          orders, no atomics, nothing read back.  ``forward_pregrouped`` stays no-grad only.
  torch   everything else -- the CPU, training without ``fused_grad``, ``fused=False`` (the benchmark's baseline): ``F.conv2d`` and
          ``F.interpolate``.

What the f8 config does not use raises ``NotImplementedError`` in the constructors.  bf16 is out of scope.  The stage maps come from the backbone of ``racformer_amd/resnet.py`` (``ResNet``), channel-first as the kernels read them."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import _lib
from .fpn_writer import cached_pack, output_conv
from .fused import (ConvImage, _scratch_ns, _zero_dgrad, conv3x3_wgrad, pack_conv3x3_dgrad_weight, pack_conv3x3_weight,
                    scratch_namespace)

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


# ------------------------------------------------------------------------------------------- backward of the lateral stage
_children = {}


def nearest_children(in_size, out_size):
    """Inverse of ``nearest_src`` along one axis: int32 CPU tensor ``start`` [in_size + 1] with ``nearest_src(d, in_size, out_size)
    == i`` exactly for ``start[i] <= d < start[i + 1]``.  src is non-decreasing in d, so the fine indices that read coarse index i are
    one contiguous range; the ranges are disjoint and cover 0 .. out_size - 1.  Same float32 arithmetic as ``nearest_src``."""
    import numpy as np
    scale = np.float32(in_size) / np.float32(out_size)
    src = np.minimum(np.floor(np.arange(out_size, dtype=np.float32) * scale).astype(np.int64), in_size - 1)
    return torch.from_numpy(np.searchsorted(src, np.arange(in_size + 1), side="left").astype(np.int32))


def _children_tables(h, w, fh, fw, device):
    """Device copies of the two range tables of a (coarse, fine) shape pair, uploaded once per shape and device."""
    key = (h, w, fh, fw, str(device))
    hit = _children.get(key)
    if hit is None:
        hit = _children[key] = (nearest_children(h, fh).to(device), nearest_children(w, fw).to(device))
    return hit


def fpn_merge_backward(a, gfine, size=None):
    """Gradient of a level's merged lateral: ``a`` [n, C, H, W] (from the level's own output convolution) or None, ``gfine``
    [n, C, fh, fw] (the finer level's merged gradient) or None -> a + the sum of gfine over each pixel's nearest-neighbour children,
    added row-major in exact float32 (rac_fpn_merge_bwd).  ``size`` = (H, W) when ``a`` is None."""
    given = [t for t in (a, gfine) if t is not None]
    if not given:
        raise RuntimeError("fpn_merge_backward: a or gfine must be given")
    _lib.require_gpu(*given, what="fpn_merge_backward")
    if any(t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous() for t in given):
        raise RuntimeError("fpn_merge_backward: contiguous float32 [n, C, H, W] tensors expected")
    if a is None and size is None:
        raise RuntimeError("fpn_merge_backward: size=(H, W) is needed when a is None")
    n, c = given[0].shape[:2]
    h, w = (int(a.shape[2]), int(a.shape[3])) if a is not None else (int(size[0]), int(size[1]))
    fh = fw = 0
    rows = cols = None
    if gfine is not None:
        if tuple(gfine.shape[:2]) != (n, c):
            raise RuntimeError("fpn_merge_backward: a and gfine must agree in images and channels")
        fh, fw = int(gfine.shape[2]), int(gfine.shape[3])
        if fh < h or fw < w:
            raise RuntimeError("fpn_merge_backward: the finer level must be at least as large as this one")
        rows, cols = _children_tables(h, w, fh, fw, gfine.device)
    out = torch.empty(n, c, h, w, device=given[0].device, dtype=torch.float32)
    opt = lambda t: _lib.ptr(t) if t is not None else None      # noqa: E731
    _lib.check(_lib.lib().rac_fpn_merge_bwd(opt(a), opt(gfine), opt(rows), opt(cols), _lib.ptr(out), n, c, h, w, fh, fw,
                                            _lib.stream_ptr()), "rac_fpn_merge_bwd")
    return out


def pack_lateral_weight_t(weight):
    """Conv2d weight [256, Cin, 1, 1] fp32 (device) -> (f16 line image of its transpose, [Cin rounded up to a multiple of 256, 8, 64],
    rows past Cin zero; 2^-s) for rac_fpn_lateral_dgrad (rac_linear_pack_wt's image); (None, None) if f16 cannot hold the weights."""
    w = weight.detach().float().reshape(weight.shape[0], -1).contiguous()
    co, cin = w.shape
    amax = float(w.abs().max())
    if co != HIP_CHANNELS or cin % 32 != 0 or not w.is_cuda or not (amax > 0.0) or amax != amax or amax == float("inf"):
        return None, None
    s = 13 - math.frexp(amax)[1] + 1          # amax * 2^s in [2^13, 2^14)
    img = torch.zeros(-(-cin // HIP_CHANNELS) * HIP_CHANNELS, co // 32, 64, device=w.device, dtype=torch.float16)
    _lib.check(_lib.lib().rac_linear_pack_wt(_lib.ptr(w), _lib.ptr(img), co, cin, float(2.0 ** s), _lib.stream_ptr()), "rac_linear_pack_wt")
    return img, 2.0 ** (-s)


def fpn_lateral_dgrad(g, packed_t, cin):
    """g float32 device [n, 256, H, W] (the merged gradient), ``packed_t`` = pack_lateral_weight_t of the level's weight ->
    [n, cin, H, W] = the gradient of the lateral convolution's input (rac_fpn_lateral_dgrad: the forward's kernel on W^T)."""
    _lib.require_gpu(g, what="fpn_lateral_dgrad")
    img, alpha = packed_t
    if img is None:
        raise RuntimeError("fpn_lateral_dgrad: weights cannot be held as f16 pairs (zero / non-finite weights)")
    if g.dtype != torch.float32 or g.dim() != 4 or g.shape[1] != HIP_CHANNELS or not g.is_contiguous():
        raise RuntimeError("fpn_lateral_dgrad: g must be contiguous float32 [n, 256, H, W]")
    if cin % 32 != 0 or tuple(img.shape) != (-(-cin // HIP_CHANNELS) * HIP_CHANNELS, HIP_CHANNELS // 32, 64):
        raise RuntimeError("fpn_lateral_dgrad: cin must match the packed transposed weight")
    n, _, h, w = g.shape
    out = torch.empty(n, cin, h, w, device=g.device, dtype=torch.float32)
    _lib.check(_lib.lib().rac_fpn_lateral_dgrad(_lib.ptr(g), _lib.ptr(img), float(alpha), _lib.ptr(out), n, cin, h, w, HIP_CHANNELS,
                                                _lib.stream_ptr()), "rac_fpn_lateral_dgrad")
    return out


def lateral_wgrad_k_splits(n, h, w, cin):
    """Number of K ranges of rac_fpn_lateral_wgrad for a shape: about 512 workgroups (two per CU) over the ci tiles (128 channels, 64
    below 128), in units of 32 pixels of one image, none empty.  A function of the shape alone: a shape always sums in the same order."""
    units = n * ((h * w + 31) // 32)
    tiles = -(-cin // (128 if cin >= 128 else 64))
    want = max(1, min(units, 512 // tiles))
    per = -(-units // want)
    return -(-units // per)


def fpn_lateral_wgrad(g, x, bias=True, k_splits=None):
    """g float32 device [n, 256, H, W], x [n, Cin, H, W] -> (dW [256, Cin, 1, 1], db [256] or None): the lateral convolution's weight
    and bias gradients (rac_fpn_lateral_wgrad: partial sums per range of pixels, added in a fixed order)."""
    _lib.require_gpu(g, x, what="fpn_lateral_wgrad")
    if any(t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous() for t in (g, x)):
        raise RuntimeError("fpn_lateral_wgrad: contiguous float32 [n, C, H, W] tensors expected")
    n, cin, h, w = x.shape
    if tuple(g.shape) != (n, HIP_CHANNELS, h, w) or n < 1:
        raise RuntimeError("fpn_lateral_wgrad: g must be [n, 256, H, W] like x, n >= 1")
    k = lateral_wgrad_k_splits(n, h, w, cin) if k_splits is None else int(k_splits)
    work = torch.empty(max(k, 1) * (HIP_CHANNELS * cin + HIP_CHANNELS), device=x.device, dtype=torch.float32)
    dw = torch.empty(HIP_CHANNELS, cin, 1, 1, device=x.device, dtype=torch.float32)
    db = torch.empty(HIP_CHANNELS, device=x.device, dtype=torch.float32) if bias else None
    _lib.check(_lib.lib().rac_fpn_lateral_wgrad(_lib.ptr(g), _lib.ptr(x), _lib.ptr(work), _lib.ptr(dw), _lib.ptr(db) if bias else None,
                                                n, cin, h, w, HIP_CHANNELS, k, _lib.stream_ptr()), "rac_fpn_lateral_wgrad")
    return dw, db


def _conv3x3_cf(img, ws, alpha):
    """rac_conv3x3_cf_fwd on a packed 256-channel image, no bias -> [n, 256, H, W] channel-first."""
    out = torch.empty(img.N, HIP_CHANNELS, img.H, img.W, device=img.dev, dtype=torch.float32)
    _lib.check(_lib.lib().rac_conv3x3_cf_fwd(_lib.ptr(img.xs), _lib.ptr(ws), None, _lib.ptr(img.amax), float(alpha), _lib.ptr(out),
                                             img.N, img.H, img.W, HIP_CHANNELS, HIP_CHANNELS, _lib.stream_ptr()), "rac_conv3x3_cf_fwd")
    return out


class _NeckCore(torch.autograd.Function):
    """A neck's HIP forward under autograd: apply(neck, *inputs, *lateral weights, *lateral biases, *output weights, *output biases) ->
    the output convolutions' results, bit for bit what the no-grad route returns.  The fp32 stage maps and merged laterals are saved,
    not the packed images (scratch shared per shape, as in ``_TemporalFusionCore``).  The backward walks the levels fine to coarse;
    per level: the 3x3 data gradient (rac_conv3x3_cf_fwd on an image of the output gradient with transposed, flipped weights), the merge
    with the finer level's gradient (rac_fpn_merge_bwd), the 3x3 weight gradient from a re-packed lateral (rac_conv3x3_wgrad), the
    lateral weight / bias gradient (rac_fpn_lateral_wgrad) and the lateral data gradient (rac_fpn_lateral_dgrad) -- each only where
    ``ctx.needs_input_grad`` asks for it or for something behind it.  The output convolutions' bias gradients are torch sums.
    Nothing is read back.  The launchers are looked up as this module's globals at call time."""

    @staticmethod
    def forward(ctx, neck, *tensors):
        L, J = len(neck.in_channels), len(neck.fpn_convs)
        inputs = [t.contiguous() for t in tensors[:L]]
        lat = neck.laterals_hip(inputs)
        outs = tuple(output_conv(lat[neck.out_levels[j]], neck._out_pack(j), neck.fpn_convs[j].conv.bias, type(neck).__name__)
                     for j in range(J))
        ctx.neck = neck
        ctx.save_for_backward(*inputs, *lat, *tensors[L:2 * L], *tensors[3 * L:3 * L + J])
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *gouts):
        neck = ctx.neck
        L, J = len(neck.in_channels), len(neck.fpn_convs)
        saved = ctx.saved_tensors
        inputs, lat, lw, ow = saved[:L], saved[L:2 * L], saved[2 * L:3 * L], saved[3 * L:3 * L + J]
        need = ctx.needs_input_grad[1:]
        need_x, need_lw, need_lb = need[:L], need[L:2 * L], need[2 * L:3 * L]
        need_ow, need_ob = need[3 * L:3 * L + J], need[3 * L + J:3 * L + 2 * J]
        gx, glw, glb, gow, gob = [None] * L, [None] * L, [None] * L, [None] * J, [None] * J
        g_fine = None
        for i in range(L):
            # the merged gradient of level i feeds its own lateral convolution and, through the top-down path, every coarser level's
            need_g = any(need_x[i:]) or any(need_lw[i:]) or any(need_lb[i:])
            a = None
            j = neck.out_levels.index(i) if i in neck.out_levels else None
            if j is not None and gouts[j] is not None and (need_g or need_ow[j] or need_ob[j]):
                go = gouts[j].contiguous()
                n, _, h, w = go.shape
                if need_g or need_ow[j]:
                    g_img = ConvImage(n, h, w, HIP_CHANNELS, go.device).begin([go]).pack(go, 0)
                if need_g:
                    ws, alpha, _ = cached_pack(neck._packs, ("fpn_dgrad", j), ow[j], pack_conv3x3_dgrad_weight)
                    a = _conv3x3_cf(g_img, ws, alpha) if ws is not None else _zero_dgrad(ow[j], go)
                if need_ow[j]:
                    # (a namespace of its own: both images are [n, H, W, 256] and would otherwise be one scratch buffer)
                    with scratch_namespace((_scratch_ns[0], "neck_lateral")):
                        x_img = ConvImage(n, h, w, HIP_CHANNELS, go.device).begin([lat[i]]).pack(lat[i], 0)
                    gow[j] = conv3x3_wgrad(x_img, g_img)
                if need_ob[j]:
                    gob[j] = go.sum(dim=(0, 2, 3))       # (torch's reduction: a fixed tree, no atomics)
            if not need_g:
                continue
            g = a if g_fine is None else fpn_merge_backward(a, g_fine, size=lat[i].shape[2:])
            g_fine = g
            if g is None:
                continue
            if need_lw[i] or need_lb[i]:
                dw, db = fpn_lateral_wgrad(g, inputs[i], bias=bool(need_lb[i]))
                glw[i], glb[i] = (dw if need_lw[i] else None), db
            if need_x[i]:
                packed = cached_pack(neck._packs, ("lateral_t", i), lw[i], pack_lateral_weight_t)
                gx[i] = fpn_lateral_dgrad(g, packed, neck.in_channels[i]) if packed[0] is not None else _zero_dgrad(lw[i], inputs[i])
        return (None, *gx, *glw, *glb, *gow, *gob)


def _refuse(name, cond, what):
    if cond:
        raise NotImplementedError(f"{name}: {what} is not used by the f8 configuration and not implemented")


class _NeckBase(nn.Module):
    """Laterals, top-down path and routing shared by the two necks; subclasses own ``fpn_convs`` and the outputs
    (``out_levels[j]``: the level whose merged lateral ``fpn_convs[j]`` reads)."""

    fused_grad = False      # opt-in: run the HIP route under autograd as well (``hip_grad_route``); off, training takes the torch route

    def __init__(self, in_channels, out_channels, fused):
        super().__init__()
        self.in_channels, self.out_channels, self.fused = list(in_channels), out_channels, fused
        self.lateral_convs = nn.ModuleList([_ConvModule(c, out_channels, 1) for c in self.in_channels])
        self.fpn_convs = nn.ModuleList()
        self._packs = {}

    def _kernels_fit(self, inputs):
        if not self.fused or self.out_channels != HIP_CHANNELS or any(c % 32 != 0 for c in self.in_channels):
            return False
        if not all(t.is_cuda and t.dtype == torch.float32 for t in inputs):
            return False
        if any(p.dtype != torch.float32 or not p.is_cuda for p in self.parameters()):
            return False
        return True

    def _records_grad(self, inputs):
        return torch.is_grad_enabled() and (any(t.requires_grad for t in inputs) or any(p.requires_grad for p in self.parameters()))

    def hip_route(self, inputs):
        """True if this call runs on the kernels without autograd (the conditions of the module docstring)."""
        return self._kernels_fit(inputs) and not self._records_grad(inputs)

    def hip_grad_route(self, inputs):
        """True if this call runs on the kernels under autograd: ``fused_grad`` is set, autograd is recording for an input or a
        parameter, and every other condition of ``hip_route`` holds (input channels up to 2048, the backward kernels' range)."""
        return bool(self.fused_grad) and self._records_grad(inputs) and self._kernels_fit(inputs) and max(self.in_channels) <= 2048

    def _forward_grad(self, inputs):
        """The HIP route under autograd: the tuple of the output convolutions' results (``_NeckCore``)."""
        lc, oc = [m.conv for m in self.lateral_convs], [m.conv for m in self.fpn_convs]
        return _NeckCore.apply(self, *inputs, *[c.weight for c in lc], *[c.bias for c in lc], *[c.weight for c in oc],
                               *[c.bias for c in oc])

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
        self.out_levels = list(range(len(self.in_channels)))

    def forward(self, inputs):
        """inputs: per level [B*T*N, C_i, H_i, W_i] -> tuple of [B*T*N, out_channels, H_i, W_i]."""
        self._check(inputs)
        if self.hip_route(inputs):
            with torch.no_grad():
                lat = self.laterals_hip(inputs)
                return tuple(output_conv(x, self._out_pack(i), self.fpn_convs[i].conv.bias, "FPN") for i, x in enumerate(lat))
        if self.hip_grad_route(inputs):
            return tuple(self._forward_grad(inputs))
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
        self.out_levels = list(self.out_ids)

    def forward(self, inputs):
        """inputs: per level [B*T*N, C_i, H_i, W_i] -> [B*T*N, out_channels, H_0, W_0], contiguous and channel-first."""
        self._check(inputs)
        if self.hip_route(inputs):
            with torch.no_grad():
                return output_conv(self.laterals_hip(inputs)[0], self._out_pack(0), self.fpn_convs[0].conv.bias, "CustomFPN")
        if self.hip_grad_route(inputs):
            return self._forward_grad(inputs)[0]
        return self.fpn_convs[0](self.laterals_torch(inputs)[0])
