"""``img_backbone`` of ``RaCFormer.extract_img_feat`` (models/racformer.py:107-126): mmdet 2.28.2's ``ResNet(depth=50,
style='pytorch', norm_eval=True)`` as configs/racformer_r50_nuimg_704x256_f8.py:67-76 builds it.  mmdet is a third-party dependency
that is not in the reference tree; this module restates it (constructor arguments, state-dict keys, ``train()``) as ``necks.FPN``
restates mmdet's FPN:

  stem      ``conv1`` 7x7 / stride 2 / pad 3 without bias, ``bn1``, ReLU, ``MaxPool2d(3, 2, 1)``
  layer1..4 (3, 4, 6, 3) Bottlenecks (depth 50), planes 64 * 2^i, strides (1, 2, 2, 2); per Bottleneck ``conv1`` 1x1, ``bn1``, ReLU,
            ``conv2`` 3x3 with the block's stride, ``bn2``, ReLU, ``conv3`` 1x1, ``bn3``, ``+ identity``, ReLU; the first block of
            every stage has ``downsample = Sequential(Conv2d 1x1 with the block's stride, BatchNorm)``

``forward`` returns one contiguous channel-first float32 ``[B*T*N, C_i, H_i, W_i]`` per member of ``out_indices``: what
``FPN.forward``, ``FPN.forward_pregrouped`` and ``CustomFPN.forward`` take, with no copy in between.  Two routes (``depth_net.py``'s
rule, ``hip_route`` tells):

  HIP     ``fused``, device float32 tensor and parameters, every BatchNorm in eval, no gradient required: ``rac_resnet_stem_fwd``
          (exact fp32 stem with the max pool) and per convolution ``rac_resnet_absmax_fwd`` + ``rac_resnet_conv_fwd``
          (csrc/resnet.hip: BatchNorm folded in float64 by ``radar_pillars.fold_bn``, split-precision f16 matrix cores at
          fp32-convolution accuracy, activation scale per image, bias / residual / ReLU in the epilogue).  No library convolution, no
          atomics, nothing read back, one stream; intermediates live in the scratch namespace in force
          (``fused.scratch_namespace``), allocated once per shape; only the returned stage maps are new tensors.  Folded and packed
          weights are cached per convolution until one of its five tensors (weight, BatchNorm affine, running statistics) changes.
  HIP, training   the same conditions with autograd recording for a parameter, the class attribute ``fused_grad`` set (opt-in,
          default False; ``hip_grad_route``), a frozen stem (``frozen_stages >= 0``) and images that need no gradient: one
          ``torch.autograd.Function`` (``_ResNetCore``) over the whole backbone.  ``norm_eval`` keeps every BatchNorm on its running
          statistics, so the forward under autograd is the folded-convolution forward above, bit for bit (``forward_hip_train``): the
          stem and every stage before the first one with a trainable parameter run on scratch as before, from that stage on each
          block's ``x, t1, t2, y`` are new tensors, saved for the backward (no scratch buffer is saved; ``with_cp`` is ignored: no
          activation checkpointing on this route).  The backward (csrc/resnet_bwd.hip; the data gradient is csrc/resnet.hip's kernel) walks the blocks last to first; per block, from
          the masked gradient ``g3`` of its output: the weight gradient of ``conv3`` from ``(g3, t2)``, ``gt2 = dgrad(conv3; mask =
          t2)``, the weight gradient and the stride-aware data gradient of ``conv2`` (``gt1``, masked by ``t1``), the weight gradient of
          ``conv1``, the identity branch (``dgrad(downsample; add = the outside gradient of the stage map below)`` and the downsample's
          weight gradient, or ``g3`` itself) and ``gx = dgrad(conv1; add = identity gradient, mask = x)``, the next block's ``g3``.
          ``rac_resnet_conv_dgrad`` carries the ReLU backward and the adds in its epilogue; ``rac_resnet_relu_bwd`` covers the
          network's last block and a stage output whose only gradient comes from outside.  ``rac_resnet_conv_wgrad`` gives the folded
          weight's and shift's gradients, ``fold_bn_backward`` (float64 torch, rounded once) turns them into those of the convolution
          weight and the BatchNorm affine.  Every launch is skipped where nothing asks for its result (frozen parameters, a ``None``
          output gradient, the data gradient into the first trainable block's input).  No atomics, fixed summation orders: two runs
          give the same bits.  Open point: ``pack_conv_weight`` / ``pack_conv_weight_t`` read the weight maximum back once per weight
          version, which in training is once per convolution and step (a device-side weight scale is not built).
  torch   everything else -- the CPU, training without ``fused_grad``, a trainable stem, images that require a gradient,
          ``fused=False`` (the timing tool's baseline): ``F.conv2d`` / ``F.batch_norm``.

``input_norm = dict(mean, std, to_rgb)`` (``data_aug['img_norm_cfg']``) makes the stem apply models/racformer.py:202-212 --
``(x[:, [2, 1, 0]] - mean) / std``, subtract and then a float32 division -- while it stages the image (no pass of its own over the
images); on the torch route the same three lines run in torch.

What the f8 configuration does not use raises ``NotImplementedError`` in the constructor: BasicBlock depths, ``style='caffe'``,
``deep_stem``, ``avg_down``, ``dcn``, ``plugins``, ``conv_cfg``, dilations, other norm types, ``in_channels != 3``.  ``with_cp`` is
accepted (ignored on the HIP route).

Out of scope: a backward for the stem and the max pool, training-mode BatchNorm (``norm_eval=False``), activation checkpointing on the
HIP route, fusing a Bottleneck's backward into fewer kernels; bf16 / fp16 storage; VoVNet and the reference's ``CustomResNet``; ``GridMask`` and the colour augmentation (training only); ``pad_multiple`` (a no-op at 256 x 704); fusing
a whole Bottleneck into one kernel; writing the necks' operands from the last block's epilogue (DESIGN.md 3.21 lists the last two as
open points)."""
import ctypes
import math

import torch
import torch.nn as nn
import torch.utils.checkpoint as cp
from torch.autograd.function import once_differentiable

from . import _lib
from . import fused as _fused
from .radar_pillars import fold_bn

ARCH = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3), 152: (3, 8, 36, 3)}
EXPANSION = 4


def _refuse(name, cond, what):
    if cond:
        raise NotImplementedError(f"{name}: {what} is not used by the f8 configuration and not implemented")


def stem_sizes(h, w):
    """(H, W) of the image -> ((Hc, Wc) after the 7x7 / 2 / 3 convolution, (Hp, Wp) after the 3x3 / 2 / 1 pool)."""
    hc, wc = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    return (hc, wc), ((hc + 2 - 3) // 2 + 1, (wc + 2 - 3) // 2 + 1)


def conv_out_size(h, w, ksize, stride):
    pad = ksize // 2
    return (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1


def conv_tile_channels(cout, images, ho, wo):
    """Output channels per workgroup of rac_resnet_conv_fwd for ``images`` output maps of ho x wo (the launcher's rule, a function of
    the shapes alone): 256 or 128 where that width divides Cout and gives every CU a workgroup (256 workgroups), 64 below.
    -> (channels, workgroups)."""
    tiles = images * ((ho * wo + 63) // 64)
    for width in (256, 128):
        if cout % width == 0 and tiles * (cout // width) >= 256:
            return width, tiles * (cout // width)
    return 64, tiles * (cout // 64)


# ------------------------------------------------------------------------------------------------------- kernels, functional
def _scratch(tag, shape, device, dtype=torch.float32):
    """A buffer of the scratch namespace in force, allocated once per (tag, shape)."""
    key = ("resnet", tag, tuple(shape), str(dtype), str(device), _fused._scratch_ns[0])
    buf = _fused._conv_images.get(key)
    if buf is None:
        buf = _fused._conv_images[key] = torch.empty(*shape, device=device, dtype=dtype)
    return buf


def pack_conv_weight(weight):
    """Folded convolution weight [Cout, Cin, k, k] fp32 (device) -> (f16 line image [Cout, k*k*Cin/32, 64] = [hi 32 | lo 32] of
    weight * 2^s with K = (tap, ci), 2^-s) for rac_resnet_conv_fwd (rac_gemm_split_pack_fwd's image)."""
    co, ci, kh, kw = weight.shape
    w = weight.detach().float().permute(0, 2, 3, 1).reshape(co, kh * kw * ci).contiguous()
    amax = float(w.abs().max())
    if ci % 32 != 0 or not w.is_cuda or amax != amax or amax == float("inf"):
        raise RuntimeError("resnet.pack_conv_weight: a device weight with Cin a multiple of 32 and finite values is needed")
    s = 13 - math.frexp(amax)[1] + 1 if amax > 0.0 else 0      # amax * 2^s in [2^13, 2^14); all-zero weights (a zero bn3.weight) stay zero
    img = torch.empty(co, kh * kw * ci // 32, 64, device=w.device, dtype=torch.float16)
    _lib.check(_lib.lib().rac_gemm_split_pack_fwd(_lib.ptr(w), _lib.ptr(img), co, kh * kw * ci, float(2.0 ** s), _lib.stream_ptr()),
               "rac_gemm_split_pack_fwd")
    return img, 2.0 ** (-s)


def pack_stem_weight(weight):
    """Folded stem weight [64, 3, 7, 7] -> f32 [147, 64], row (ci * 7 + ky) * 7 + kx (rac_resnet_stem_fwd's w)."""
    return weight.detach().float().permute(1, 2, 3, 0).reshape(147, 64).contiguous()


def image_absmax(x, parts=None):
    """x float32 device [n, ...] -> [n, 64] partial maxima of |x| per image (rac_resnet_absmax_fwd)."""
    n = x.shape[0]
    if parts is None:
        parts = torch.empty(n, _lib.RESNET_AMAX_PARTS, device=x.device, dtype=torch.float32)
    _lib.check(_lib.lib().rac_resnet_absmax_fwd(_lib.ptr(x), _lib.ptr(parts), n, x.numel() // n, _lib.stream_ptr()), "rac_resnet_absmax_fwd")
    return parts


def conv_fwd(x, packed, bias, ksize, stride, residual=None, relu=True, out=None, parts=None):
    """x float32 device [n, Cin, H, W], ``packed`` = pack_conv_weight of the folded weight, bias [Cout] or None, residual
    [n, Cout, Ho, Wo] or None -> [n, Cout, Ho, Wo] = [relu](conv(x) + bias [+ residual]) (rac_resnet_absmax_fwd unless ``parts`` is
    given, then rac_resnet_conv_fwd)."""
    _lib.require_gpu(x, *([residual] if residual is not None else []), what="resnet.conv_fwd")
    n, cin, h, w = x.shape
    img, alpha = packed
    cout = img.shape[0]
    ho, wo = conv_out_size(h, w, ksize, stride)
    if x.dtype != torch.float32 or img.shape[1] * 32 != ksize * ksize * cin:
        raise RuntimeError("resnet.conv_fwd: x must be float32 [n, Cin, H, W] with Cin and ksize matching the packed weight")
    if residual is not None and (residual.dtype != torch.float32 or tuple(residual.shape) != (n, cout, ho, wo)):
        raise RuntimeError("resnet.conv_fwd: residual must be float32 [n, Cout, Ho, Wo]")
    if parts is None:
        parts = image_absmax(x)
    if out is None:
        out = torch.empty(n, cout, ho, wo, device=x.device, dtype=torch.float32)
    d = _lib.ResnetConv(_lib.ptr(x), _lib.ptr(img), _lib.ptr(bias) if bias is not None else None,
                        _lib.ptr(residual) if residual is not None else None, _lib.ptr(parts), _lib.ptr(out), float(alpha),
                        n, h, w, cin, cout, ksize, stride, int(bool(relu)))
    _lib.check(_lib.lib().rac_resnet_conv_fwd(ctypes.byref(d), _lib.stream_ptr()), "rac_resnet_conv_fwd")
    return out


# ------------------------------------------------------------------------------------------------------- backward, functional
def conv_wgrad_k_splits(n, ho, wo, cin, cout, ksize):
    """Number of K ranges of rac_resnet_conv_wgrad for a shape (n images, output map ho x wo): about 512 workgroups (two per CU) over
    the taps and the launcher's tiles (128 co x 128 ci where Cout is a multiple of 128 and Cin at least 128, 64 x 64 below), in units of
    32 output pixels of one image, none empty.  A function of the shape alone: a shape always sums in the same order."""
    units = n * ((ho * wo + 31) // 32)
    tile = 128 if cout % 128 == 0 and cin >= 128 else 64
    tiles = ksize * ksize * (cout // tile) * (-(-cin // tile))
    want = max(1, min(units, 512 // tiles))
    per = -(-units // want)
    return -(-units // per)


def pack_conv_weight_t(weight):
    """Folded convolution weight [Cout, Cin, k, k] fp32 (device) -> (f16 line image [Cin, k*k*Cout/32, 64] of its transpose with the
    taps flipped, K = (flipped tap, co), times 2^s; 2^-s) for rac_resnet_conv_dgrad (rac_gemm_split_pack_fwd's image)."""
    co, ci, kh, kw = weight.shape
    w = weight.detach().float().flip(2, 3).permute(1, 2, 3, 0).reshape(ci, kh * kw * co).contiguous()
    amax = float(w.abs().max())
    if co % 32 != 0 or not w.is_cuda or amax != amax or amax == float("inf"):
        raise RuntimeError("resnet.pack_conv_weight_t: a device weight with Cout a multiple of 32 and finite values is needed")
    s = 13 - math.frexp(amax)[1] + 1 if amax > 0.0 else 0
    img = torch.empty(ci, kh * kw * co // 32, 64, device=w.device, dtype=torch.float16)
    _lib.check(_lib.lib().rac_gemm_split_pack_fwd(_lib.ptr(w), _lib.ptr(img), ci, kh * kw * co, float(2.0 ** s), _lib.stream_ptr()),
               "rac_gemm_split_pack_fwd")
    return img, 2.0 ** (-s)


def _grad_maps(what, *tensors):
    _lib.require_gpu(*tensors, what=what)
    if any(t.dtype != torch.float32 or t.dim() != 4 for t in tensors):
        raise RuntimeError(f"{what}: contiguous float32 [n, C, H, W] tensors expected")


def conv_dgrad(g, packed_t, ksize, stride, size, add=None, mask=None, parts=None):
    """g float32 device [n, Cout, Ho, Wo] (the gradient of a convolution's output), ``packed_t`` = pack_conv_weight_t of its folded
    weight, ``size`` = (H, W) of the convolution's input -> [n, Cin, H, W] = the gradient of that input [+ add], zero where
    ``mask <= 0`` (rac_resnet_absmax_fwd of g unless ``parts`` is given, then rac_resnet_conv_dgrad)."""
    extra = [t for t in (add, mask) if t is not None]
    _grad_maps("resnet.conv_dgrad", g, *extra)
    n, cout, ho, wo = g.shape
    h, w = int(size[0]), int(size[1])
    img, alpha = packed_t
    cin = img.shape[0]
    if img.shape[1] * 32 != ksize * ksize * cout or conv_out_size(h, w, ksize, stride) != (ho, wo):
        raise RuntimeError("resnet.conv_dgrad: g must be [n, Cout, Ho, Wo] of the packed weight's convolution on an H x W input")
    if any(tuple(t.shape) != (n, cin, h, w) for t in extra):
        raise RuntimeError("resnet.conv_dgrad: add and mask must be float32 [n, Cin, H, W]")
    if parts is None:
        parts = image_absmax(g)
    out = torch.empty(n, cin, h, w, device=g.device, dtype=torch.float32)
    d = _lib.ResnetDgrad(_lib.ptr(g), _lib.ptr(img), _lib.ptr(add) if add is not None else None,
                         _lib.ptr(mask) if mask is not None else None, _lib.ptr(parts), _lib.ptr(out), float(alpha), n, h, w, ho, wo,
                         cin, cout, ksize, stride)
    _lib.check(_lib.lib().rac_resnet_conv_dgrad(ctypes.byref(d), _lib.stream_ptr()), "rac_resnet_conv_dgrad")
    return out


def conv_wgrad(g, x, ksize, stride, bias=True, k_splits=None):
    """g float32 device [n, Cout, Ho, Wo], x [n, Cin, H, W] (the convolution's input) -> (dW [Cout, Cin, k, k], db [Cout] or None): the
    gradients of the folded weight and shift (rac_resnet_conv_wgrad: partial sums per range of pixels, added in a fixed order)."""
    _grad_maps("resnet.conv_wgrad", g, x)
    n, cin, h, w = x.shape
    cout, ho, wo = g.shape[1:]
    if g.shape[0] != n or conv_out_size(h, w, ksize, stride) != (ho, wo):
        raise RuntimeError("resnet.conv_wgrad: g must be [n, Cout, Ho, Wo] of the convolution of x")
    k = conv_wgrad_k_splits(n, ho, wo, cin, cout, ksize) if k_splits is None else int(k_splits)
    work = torch.empty(max(k, 1) * (ksize * ksize * cout * cin + cout), device=x.device, dtype=torch.float32)
    dw = torch.empty(cout, cin, ksize, ksize, device=x.device, dtype=torch.float32)
    db = torch.empty(cout, device=x.device, dtype=torch.float32) if bias else None
    _lib.check(_lib.lib().rac_resnet_conv_wgrad(_lib.ptr(g), _lib.ptr(x), _lib.ptr(work), _lib.ptr(dw), _lib.ptr(db) if bias else None,
                                                n, cin, h, w, cout, ho, wo, ksize, stride, k, _lib.stream_ptr()), "rac_resnet_conv_wgrad")
    return dw, db


def relu_bwd(y, a, b=None):
    """y, a[, b] float32 device tensors of one shape -> where(y > 0, a [+ b], 0) (rac_resnet_relu_bwd)."""
    given = [t for t in (y, a, b) if t is not None]
    _lib.require_gpu(*given, what="resnet.relu_bwd")
    if any(t.dtype != torch.float32 or t.shape != y.shape for t in given) or y.numel() < 1:
        raise RuntimeError("resnet.relu_bwd: non-empty float32 tensors of one shape expected")
    out = torch.empty_like(y)
    _lib.check(_lib.lib().rac_resnet_relu_bwd(_lib.ptr(y), _lib.ptr(a), _lib.ptr(b) if b is not None else None, _lib.ptr(out),
                                              y.numel(), _lib.stream_ptr()), "rac_resnet_relu_bwd")
    return out


def fold_bn_backward(dw_folded, db_folded, weight, bn, need=None):
    """Backward of ``fold_bn``: the gradients of the folded weight W' = W * s and shift b' = beta - mean * s (s = gamma / sqrt(var +
    eps)) -> (dW, dgamma, dbeta) = (dW' * s, (sum_{ci,ky,kx} dW' * W - mean * db') / sqrt(var + eps), db'), in float64, rounded to
    float32 once.  Only what requires a gradient is computed (``need`` = three flags; default: the tensors' ``requires_grad``), the
    rest is None; ``db_folded`` may be None where neither BatchNorm gradient is needed."""
    nw, ng, nb = (weight.requires_grad, bn.weight.requires_grad, bn.bias.requires_grad) if need is None else need
    inv = 1.0 / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    dw = dgamma = dbeta = None
    if nw:
        s = bn.weight.detach().double() * inv
        dw = (dw_folded.double() * s.view(-1, 1, 1, 1)).float()
    if ng:
        dot = (dw_folded.double() * weight.detach().double()).sum(dim=(1, 2, 3))
        dgamma = ((dot - bn.running_mean.detach().double() * db_folded.double()) * inv).float()
    if nb:
        dbeta = db_folded.double().float()
    return dw, dgamma, dbeta


def trainable_blocks(model):
    """[(stage, block)] of every Bottleneck from the first stage with a parameter that requires a gradient on, in forward order."""
    stages = [getattr(model, name) for name in model.res_layers]
    first = next((i for i, st in enumerate(stages) if any(p.requires_grad for p in st.parameters())), len(stages))
    return [(i, b) for i in range(first, len(stages)) for b in range(len(stages[i]))]


def forward_hip_train(model, x):
    """The HIP forward as the autograd route runs it: x [n, 3, H, W] -> (outs, saved).  ``outs``: the ``out_indices`` stage maps, bit
    for bit ``forward_hip``'s.  ``saved``: one ``(x, t1, t2, y)`` per block of ``trainable_blocks(model)``, in forward order -- the
    block's input, its two post-ReLU intermediates and its post-ReLU output, all new tensors (a block's ``y`` is the next block's
    ``x``); the backward takes its ReLU decisions from them.  The stem and the stages before run on scratch."""
    _lib.require_gpu(x.contiguous(), what="ResNet")
    blocks = trainable_blocks(model)
    first = blocks[0][0] if blocks else len(model.res_layers)
    h = model.stem_hip(x)
    outs, saved = [], []
    for i in range(len(model.res_layers)):
        if i < first:
            h = model.stage_hip(i, h)
        else:
            if i == first and (i == 0 or i - 1 not in model.out_indices):
                h = h.clone()                    # (the stage's input is scratch: the backward reads it long after)
            for b in range(len(getattr(model, model.res_layers[i]))):
                h = model.block_hip(i, b, h, save=saved)
        if i in model.out_indices:
            outs.append(h)
    return tuple(outs), saved


class _ResNetCore(torch.autograd.Function):
    """The backbone's HIP forward under autograd: apply(model, x, *(conv.weight, bn.weight, bn.bias per convolution of
    ``trainable_blocks``, in ``Bottleneck.convs()`` order)) -> the ``out_indices`` stage maps, bit for bit the no-grad route's.  Saved:
    ``forward_hip_train``'s tensors (the parameters and running statistics are read from the modules).  The backward walks the blocks last to first (module docstring); each launch
    runs only where ``ctx.needs_input_grad`` asks for its result or for something behind it; a ``None`` output gradient adds nothing.
    Nothing is read back but the weight maxima of the transposed packs (once per weight version).  The launchers are looked up as
    this module's globals at call time."""

    @staticmethod
    def forward(ctx, model, x, *params):
        outs, saved = forward_hip_train(model, x)
        ctx.model, ctx.blocks = model, trainable_blocks(model)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*[t for blk in saved for t in blk])
        first = ctx.blocks[0][0]
        stages = [i for i in range(len(model.res_layers)) if i in model.out_indices]
        ctx.mark_non_differentiable(*[o for o, i in zip(outs, stages) if i < first])      # (as on the torch route: frozen stages)
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *gouts):
        model, blocks = ctx.model, ctx.blocks
        saved = [ctx.saved_tensors[4 * k:4 * k + 4] for k in range(len(blocks))]
        flags = ctx.needs_input_grad[2:]
        # per block: {convolution name: (position of its three parameters, the three flags)}
        need, pos = [], 0
        for i, b in blocks:
            per = {}
            for name, _, _ in getattr(model, model.res_layers[i])[b].convs():
                per[name] = (pos, tuple(flags[pos:pos + 3]))
                pos += 3
            need.append(per)
        grads = [None] * pos
        wanted = [k for k, per in enumerate(need) if any(any(f) for _, f in per.values())]
        if not wanted:
            return (None, None, *grads)
        first = wanted[0]
        outside = {}                                              # stage -> its map's gradient from outside, or None
        for j, i in enumerate(i for i in range(len(model.res_layers)) if i in model.out_indices):
            outside[i] = gouts[j].contiguous() if gouts[j] is not None else None

        def below(k):
            """the outside gradient of block k's input, if that is a stage map"""
            i, b = blocks[k]
            return outside.get(i - 1) if b == 0 else None

        def conv_of(k, name):
            i, b = blocks[k]
            return next((c, m) for n, c, m in getattr(model, model.res_layers[i])[b].convs() if n == name)

        def param_grads(k, name, g, xin, ksize, stride):
            at, (nw, ng, nb) = need[k][name]
            if not (nw or ng or nb):
                return
            conv, bn = conv_of(k, name)
            dw, db = conv_wgrad(g, xin, ksize, stride, bias=bool(ng or nb))
            grads[at:at + 3] = fold_bn_backward(dw, db, conv.weight, bn, (nw, ng, nb))

        def packed_t(k, name):
            return model._pack(blocks[k] + (name, "t"), *conv_of(k, name), pack_conv_weight_t)[0]

        top = outside.get(blocks[-1][0])
        g3 = relu_bwd(saved[-1][3], top) if top is not None else None
        for k in range(len(blocks) - 1, first - 1, -1):
            i, b = blocks[k]
            blk = getattr(model, model.res_layers[i])[b]
            x, t1, t2, y = saved[k]
            need_dx = k > first
            if g3 is None:
                # nothing arrives from above: the block's input may still be a stage map with a gradient of its own
                if need_dx and below(k) is not None:
                    g3 = relu_bwd(x, below(k))
                continue
            n1, n2 = any(need[k]["conv1"][1]), any(need[k]["conv2"][1])
            param_grads(k, "conv3", g3, t2, 1, 1)
            parts3 = image_absmax(g3) if (need_dx or n1 or n2) else None
            gt1 = None
            if need_dx or n1 or n2:
                gt2 = conv_dgrad(g3, packed_t(k, "conv3"), 1, 1, t2.shape[2:], mask=t2, parts=parts3)
                param_grads(k, "conv2", gt2, t1, 3, blk.stride)
                if need_dx or n1:
                    gt1 = conv_dgrad(gt2, packed_t(k, "conv2"), 3, blk.stride, t1.shape[2:], mask=t1)
                    param_grads(k, "conv1", gt1, x, 1, 1)
            if blk.downsample is not None:
                param_grads(k, "downsample", g3, x, 1, blk.stride)
            if not need_dx:
                break
            if blk.downsample is not None:
                gid = conv_dgrad(g3, packed_t(k, "downsample"), 1, blk.stride, x.shape[2:], add=below(k), parts=parts3)
            else:
                if below(k) is not None:
                    raise RuntimeError("ResNet: a stage whose first block has no downsample is not supported by the HIP backward")
                gid = g3
            g3 = conv_dgrad(gt1, packed_t(k, "conv1"), 1, 1, x.shape[2:], add=gid, mask=x)
        return (None, None, *grads)


def norm_args(input_norm):
    """``input_norm`` -> (perm, mean, std) lists of three, or None."""
    if input_norm is None:
        return None
    mean, std = [float(v) for v in input_norm['mean']], [float(v) for v in input_norm['std']]
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("ResNet.input_norm: mean and std of three channels expected")
    return ([2, 1, 0] if input_norm.get('to_rgb', False) else [0, 1, 2]), mean, std


def stem_fwd(x, w147, bias, input_norm=None, out=None):
    """x float32 device [n, 3, H, W], w147 = pack_stem_weight of the folded weight, bias [64] -> [n, 64, Hp, Wp] after convolution,
    ReLU and max pool (rac_resnet_stem_fwd); the convolution's own output is scratch of the namespace in force."""
    _lib.require_gpu(x, what="resnet.stem_fwd")
    n, c, h, w = x.shape
    if c != 3 or x.dtype != torch.float32:
        raise RuntimeError("resnet.stem_fwd: x must be float32 [n, 3, H, W]")
    (hc, wc), (hp, wp) = stem_sizes(h, w)
    conv = _scratch("stem_conv", (n, 64, hc, wc), x.device)
    if out is None:
        out = torch.empty(n, 64, hp, wp, device=x.device, dtype=torch.float32)
    na = norm_args(input_norm)
    perm, mean, std = na if na is not None else ([0, 1, 2], [0.0] * 3, [1.0] * 3)
    d = _lib.ResnetStem(_lib.ptr(x), _lib.ptr(w147), _lib.ptr(bias), _lib.ptr(conv), _lib.ptr(out), n, h, w, int(na is not None),
                        (ctypes.c_int * 3)(*perm), (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std))
    _lib.check(_lib.lib().rac_resnet_stem_fwd(ctypes.byref(d), _lib.stream_ptr()), "rac_resnet_stem_fwd")
    return out


def apply_input_norm(x, input_norm):
    """models/racformer.py:202-212 in torch."""
    perm, mean, std = norm_args(input_norm)
    if perm != [0, 1, 2]:
        x = x[:, perm, :, :]
    x = x - torch.tensor(mean, device=x.device, dtype=x.dtype).reshape(1, 3, 1, 1)
    return x / torch.tensor(std, device=x.device, dtype=x.dtype).reshape(1, 3, 1, 1)


# ----------------------------------------------------------------------------------------------------------------- modules
class Bottleneck(nn.Module):
    """mmdet's Bottleneck, style 'pytorch' (the stride sits on ``conv2``)."""
    expansion = EXPANSION

    def __init__(self, inplanes, planes, stride=1, downsample=None, with_cp=False):
        super().__init__()
        self.inplanes, self.planes, self.stride, self.with_cp = inplanes, planes, stride, with_cp
        self.conv1 = nn.Conv2d(inplanes, planes, 1, stride=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * EXPANSION, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * EXPANSION)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    def forward(self, x):
        def inner(x):
            out = self.relu(self.bn1(self.conv1(x)))
            out = self.relu(self.bn2(self.conv2(out)))
            out = self.bn3(self.conv3(out))
            return out + (x if self.downsample is None else self.downsample(x))

        out = cp.checkpoint(inner, x) if self.with_cp and x.requires_grad else inner(x)
        return self.relu(out)

    def convs(self):
        """(name, conv, bn) of this block's convolutions in launch order."""
        out = [("conv1", self.conv1, self.bn1), ("conv2", self.conv2, self.bn2), ("conv3", self.conv3, self.bn3)]
        if self.downsample is not None:
            out.append(("downsample", self.downsample[0], self.downsample[1]))
        return out


class ResNet(nn.Module):
    """mmdet 2.28.2's ``ResNet`` for the Bottleneck depths, with its constructor arguments, defaults and state-dict keys
    (``conv1.weight``, ``bn1.*``, ``layer{s}.{b}.conv{1,2,3}.weight``, ``layer{s}.{b}.bn{1,2,3}.*``,
    ``layer{s}.{b}.downsample.{0.weight,1.*}``), plus ``fused`` and the attributes ``input_norm`` and ``fused_grad`` (module
    docstring)."""

    fused_grad = False      # opt-in: run the HIP route under autograd as well (``hip_grad_route``); off, training takes the torch route

    def __init__(self, depth, in_channels=3, stem_channels=None, base_channels=64, num_stages=4, strides=(1, 2, 2, 2),
                 dilations=(1, 1, 1, 1), out_indices=(0, 1, 2, 3), style='pytorch', deep_stem=False, avg_down=False, frozen_stages=-1,
                 conv_cfg=None, norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), plugins=None, with_cp=False, zero_init_residual=True, pretrained=None,
                 init_cfg=None, fused=True):
        _refuse("ResNet", depth in (18, 34), "a BasicBlock depth (18, 34)")
        if depth not in ARCH:
            raise KeyError(f"invalid depth {depth} for resnet")
        _refuse("ResNet", style != 'pytorch', "style='caffe'")
        _refuse("ResNet", bool(deep_stem), "deep_stem")
        _refuse("ResNet", bool(avg_down), "avg_down")
        _refuse("ResNet", dcn is not None or any(stage_with_dcn), "dcn / stage_with_dcn")
        _refuse("ResNet", plugins is not None, "plugins")
        _refuse("ResNet", conv_cfg is not None, "conv_cfg")
        _refuse("ResNet", any(d != 1 for d in dilations), "a dilation other than 1")
        _refuse("ResNet", dict(norm_cfg).get('type') not in ('BN', 'BN2d'), "a norm type other than BN / BN2d")
        _refuse("ResNet", in_channels != 3, "in_channels != 3")
        if not 1 <= num_stages <= 4 or len(strides) < num_stages or len(dilations) < num_stages or max(out_indices) >= num_stages:
            raise ValueError("ResNet: num_stages in 1..4, one stride and dilation per stage, out_indices below num_stages")
        super().__init__()
        self.depth, self.in_channels, self.base_channels, self.num_stages = depth, in_channels, base_channels, num_stages
        self.stem_channels = stem_channels = base_channels if stem_channels is None else stem_channels
        self.strides, self.dilations, self.out_indices = tuple(strides), tuple(dilations), tuple(out_indices)
        self.style, self.frozen_stages, self.norm_cfg, self.norm_eval = style, frozen_stages, dict(norm_cfg), norm_eval
        self.with_cp, self.zero_init_residual, self.pretrained, self.init_cfg = with_cp, zero_init_residual, pretrained, init_cfg
        self.fused, self.input_norm = fused, None
        self.stage_blocks = ARCH[depth][:num_stages]

        self.conv1 = nn.Conv2d(in_channels, stem_channels, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(stem_channels)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.res_layers, inplanes = [], stem_channels
        for i, blocks in enumerate(self.stage_blocks):
            planes, stride, layer = base_channels * 2 ** i, self.strides[i], []
            for b in range(blocks):
                down = None
                if b == 0 and (stride != 1 or inplanes != planes * EXPANSION):
                    down = nn.Sequential(nn.Conv2d(inplanes, planes * EXPANSION, 1, stride=stride, bias=False),
                                         nn.BatchNorm2d(planes * EXPANSION))
                layer.append(Bottleneck(inplanes, planes, stride if b == 0 else 1, down, with_cp))
                inplanes = planes * EXPANSION
            self.add_module(f"layer{i + 1}", nn.Sequential(*layer))
            self.res_layers.append(f"layer{i + 1}")
        self.feat_dim = inplanes
        if not self.norm_cfg.get('requires_grad', True):
            for m in self.modules():
                if isinstance(m, nn.BatchNorm2d):
                    for p in m.parameters():
                        p.requires_grad = False
        self._packs = {}
        self._freeze_stages()

    # ------------------------------------------------------------------------------------------------------- mmdet's behaviour
    def init_weights(self):
        """mmdet's default initialisation: Kaiming-normal convolutions, unit BatchNorms, a zero ``bn3.weight`` per block with
        ``zero_init_residual`` (checkpoints are loaded with ``load_state_dict``: ``pretrained`` / ``init_cfg`` are kept, not read)."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1.0)
                nn.init.constant_(m.bias, 0.0)
        if self.zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.constant_(m.bn3.weight, 0.0)

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.bn1.eval()
            for m in (self.conv1, self.bn1):
                for p in m.parameters():
                    p.requires_grad = False
        for i in range(1, self.frozen_stages + 1):
            if i > len(self.res_layers):
                break
            m = getattr(self, f"layer{i}")
            m.eval()
            for p in m.parameters():
                p.requires_grad = False

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        if mode and self.norm_eval:
            for m in self.modules():
                if isinstance(m, nn.modules.batchnorm._BatchNorm):
                    m.eval()
        return self

    # ------------------------------------------------------------------------------------------------------------------ routes
    def _kernels_fit(self, x):
        """The conditions of both HIP routes that have nothing to do with gradients."""
        if not self.fused or self.stem_channels != 64 or self.base_channels % 64 != 0 or self.feat_dim > 2048:
            return False
        if any(s not in (1, 2) for s in self.strides[:self.num_stages]):
            return False
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.shape[1] == 3 and x.shape[0] >= 1):
            return False
        if any(p.dtype != torch.float32 or not p.is_cuda for p in self.parameters()):
            return False
        if any(m.training for m in self.modules() if isinstance(m, nn.modules.batchnorm._BatchNorm)):
            return False
        return True

    def hip_route(self, x):
        """True if this call runs on the kernels (the conditions of the module docstring)."""
        if not self._kernels_fit(x):
            return False
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            return False
        return True

    def hip_grad_route(self, x):
        """True if this call runs on the kernels under autograd: ``fused_grad``, the kernels fit, autograd records for a parameter, the
        stem is frozen and the images need no gradient."""
        if not self.fused_grad:
            return False
        if not self._kernels_fit(x) or not torch.is_grad_enabled() or x.requires_grad or self.frozen_stages < 0:
            return False
        if any(p.requires_grad for m in (self.conv1, self.bn1) for p in m.parameters()):
            return False
        return any(p.requires_grad for p in self.parameters())

    def forward(self, x):
        """x [B*T*N, 3, H, W] -> tuple of [B*T*N, C_i, H_i, W_i], one per member of ``out_indices``."""
        if self.hip_route(x):
            with torch.no_grad():
                return self.forward_hip(x)
        if self.hip_grad_route(x):
            params = [p for i, b in trainable_blocks(self) for _, conv, bn in getattr(self, self.res_layers[i])[b].convs()
                      for p in (conv.weight, bn.weight, bn.bias)]
            return _ResNetCore.apply(self, x, *params)
        if self.input_norm is not None:
            x = apply_input_norm(x, self.input_norm)
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        outs = []
        for i, name in enumerate(self.res_layers):
            x = getattr(self, name)(x)
            if i in self.out_indices:
                outs.append(x.contiguous())
        return tuple(outs)

    # --------------------------------------------------------------------------------------------------------------- HIP route
    def _pack(self, key, conv, bn, packer=None):
        """Folded and packed operands of one convolution, kept until one of its five tensors is replaced, written in place or moved.
        ``packer``: the packing of the folded weight (default: the forward's)."""
        tensors = (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)
        sig = tuple((t.data_ptr(), t._version, str(t.device)) for t in tensors)
        hit = self._packs.get(key)
        if hit is None or hit[0] != sig:
            with torch.no_grad():
                w, shift = fold_bn(conv.weight, bn)
                if packer is None:
                    packer = pack_stem_weight if key == "stem" else pack_conv_weight
                hit = self._packs[key] = (sig, (packer(w), shift))
        return hit[1]

    def stem_hip(self, x):
        """The stem on the kernels: [n, 3, H, W] -> scratch [n, 64, Hp, Wp]."""
        x = x.contiguous()
        w147, bias = self._pack("stem", self.conv1, self.bn1)
        (_, _), (hp, wp) = stem_sizes(x.shape[2], x.shape[3])
        return stem_fwd(x, w147, bias, self.input_norm, out=_scratch("stem_out", (x.shape[0], 64, hp, wp), x.device))

    def block_hip(self, i, b, x, out=None, save=None):
        """Bottleneck b of stage i on the kernels: three or four convolutions, each behind the per-image maximum of its input.
        ``out`` None: a new tensor.  ``save``: a list that receives ``(x, t1, t2, y)``, the two intermediates then new tensors too."""
        blk = getattr(self, self.res_layers[i])[b]
        n, dev = x.shape[0], x.device
        parts = _scratch("amax", (n, _lib.RESNET_AMAX_PARTS), dev)
        pk = {name: self._pack((i, b, name), conv, bn) for name, conv, bn in blk.convs()}
        h, w = x.shape[2], x.shape[3]
        ho, wo = conv_out_size(h, w, 3, blk.stride)
        image_absmax(x, parts)
        keep = save is not None
        t1 = conv_fwd(x, *pk["conv1"], 1, 1, out=None if keep else _scratch("t1", (n, blk.planes, h, w), dev), parts=parts)
        identity = x
        if blk.downsample is not None:
            identity = conv_fwd(x, *pk["downsample"], 1, blk.stride, relu=False,
                                out=_scratch("down", (n, blk.planes * EXPANSION, ho, wo), dev), parts=parts)
        image_absmax(t1, parts)
        t2 = conv_fwd(t1, *pk["conv2"], 3, blk.stride, out=None if keep else _scratch("t2", (n, blk.planes, ho, wo), dev), parts=parts)
        image_absmax(t2, parts)
        if out is None:
            out = torch.empty(n, blk.planes * EXPANSION, ho, wo, device=dev, dtype=torch.float32)
        y = conv_fwd(t2, *pk["conv3"], 1, 1, residual=identity, out=out, parts=parts)
        if keep:
            save.append((x, t1, t2, y))
        return y

    def stage_hip(self, i, x):
        """Stage i (``layer{i + 1}``) on the kernels; the result is a new tensor if i is in ``out_indices``, scratch otherwise.  Block
        outputs alternate between two scratch buffers: a block's input, its identity, lives until its last convolution."""
        blocks = getattr(self, self.res_layers[i])
        for b, blk in enumerate(blocks):
            out = None
            if b < len(blocks) - 1 or i not in self.out_indices:
                ho, wo = conv_out_size(x.shape[2], x.shape[3], 3, blk.stride)
                out = _scratch(("block", b & 1), (x.shape[0], blk.planes * EXPANSION, ho, wo), x.device)
            x = self.block_hip(i, b, x, out)
        return x

    def forward_hip(self, x):
        _lib.require_gpu(x.contiguous(), what="ResNet")
        x = self.stem_hip(x)
        outs = []
        for i in range(len(self.res_layers)):
            x = self.stage_hip(i, x)
            if i in self.out_indices:
                outs.append(x)
        return tuple(outs)
