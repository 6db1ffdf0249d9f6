"""Drop-in for the reference's ``models/csrc/wrapper.py`` (msmv sampling operator surface):
``msmv_sampling``, ``MSMVSamplingC2345/C45/C23456`` and the ``MSMV_CUDA`` flag, on top of
``rac_msmv_fwd`` (hand-written HIP, racformer_amd/csrc/msmv_fwd.hip).

Same names, argument meaning and error behaviour as the reference (wrapper.py:78-153,
msmv_sampling.cpp:132-184): features channel-last ``[B', N, H, W, C]``, contiguous device tensors,
``RuntimeError`` on non-contiguous / non-device inputs and on ``P > 128``; the result is a new
``[B', Q, C, P]`` float32 tensor.  ``backward`` runs rac_msmv_bwd (fp32 features).

``msmv_sampling_v2`` (wrapper.py:41-76, used by sampling_4d(aggregate=False)) samples each point on the level with the
largest scale weight only, unweighted, on top of ``rac_msmv_v2_fwd`` / ``rac_msmv_v2_bwd`` (csrc/msmv_v2.hip).
"""
import ctypes

import torch

from . import _lib

MSMV_CUDA = True  # the HIP operator is the only path; there is no torch fallback in this package


def msmv_forward(mlvl_feats, sampling_locations, scale_weights, out_layout=_lib.OUT_SQCP,
                 num_frames=1, num_groups=1, out=None):
    """Launches rac_msmv_fwd on the current stream.  ``out_layout=OUT_BQGTPC`` writes
    ``[B, Q, G, T*P, C]`` directly (what sampling_4d returns, sparsebev_sampling.py:128-131)."""
    feats = list(mlvl_feats)
    L = len(feats)
    _lib.require_gpu(*feats, sampling_locations, scale_weights, what="msmv_sampling")
    S, N, C, Q, P = _shapes(feats, sampling_locations, scale_weights, False, "msmv_sampling")
    code = _lib.dtype_code(feats[0])
    if out is None:
        out = torch.empty(_out_shape(out_layout, S, Q, C, P, num_frames, num_groups),
                          device=feats[0].device, dtype=torch.float32)
    ptrs, hw = _levels(feats, False)
    ev = _lib.timer.record("msmv_fwd") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    rc = _lib.lib().rac_msmv_fwd(ptrs, hw, L, _lib.ptr(sampling_locations), _lib.ptr(scale_weights),
                                 _lib.ptr(out), S, N, Q, P, C, code, out_layout, num_frames, num_groups,
                                 _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_msmv_fwd")
    if _lib.timer is not None and getattr(_lib.timer, "capture_inputs", False):
        _lib.timer.captured.append((sampling_locations.detach(), [tuple(f.shape) for f in feats]))
    return out


def _shapes(feats, sampling_locations, scale_weights, channels_first, what):
    """-> (S, N, C, Q, P) of a call, raising the RuntimeErrors of the reference's wrapper on inconsistent operands.
    Features channel-last ``[B', N, H, W, C]`` or, ``channels_first``, ``[B', C, N, H, W]``."""
    L = len(feats)
    if any(f.dim() != 5 for f in feats):
        raise RuntimeError(f"{what}: features must be 5-d")
    if channels_first:
        S, C, N = feats[0].shape[:3]
    else:
        S, N, _, _, C = feats[0].shape
    _, Q, P, three = sampling_locations.shape
    if three != 3 or sampling_locations.shape[0] != S:
        raise RuntimeError(f"{what}: sampling_locations must be [B', Q, P, 3]")
    if tuple(scale_weights.shape) != (S, Q, P, L):
        raise RuntimeError(f"{what}: scale_weights must be [B', Q, P, {L}], got {tuple(scale_weights.shape)}")
    if P > 128:
        raise RuntimeError("num_point exceed limits")
    for f in feats:
        lead = (f.shape[0], f.shape[1], f.shape[2]) if channels_first else (f.shape[0], f.shape[1], f.shape[4])
        if f.dtype != feats[0].dtype or lead != ((S, C, N) if channels_first else (S, N, C)):
            layout = "[B', C, N, ., .]" if channels_first else "[B', N, ., ., C]"
            raise RuntimeError(f"{what}: all levels must share dtype and {layout}")
    if sampling_locations.dtype != torch.float32 or scale_weights.dtype != torch.float32:
        raise RuntimeError(f"{what}: locations / weights must be float32")
    return S, N, C, Q, P


def _out_shape(layout, S, Q, C, P, num_frames, num_groups):
    """the forward's output shape in ``layout``: [B', Q, C, P], or [B, Q, G, T*P, C] for OUT_BQGTPC"""
    if layout == _lib.OUT_SQCP:
        return (S, Q, C, P)
    return (S // (num_frames * num_groups), Q, num_groups, num_frames * P, C)


def _grad_shape(grad_layout, S, Q, C, P, num_frames, num_groups, what):
    """the shape a gradient in ``grad_layout`` must have (the forward's output shape in that layout)"""
    if grad_layout not in (_lib.OUT_SQCP, _lib.OUT_BQGTPC):
        raise RuntimeError(f"{what}: unknown gradient layout {grad_layout}")
    if grad_layout == _lib.OUT_BQGTPC and (num_frames < 1 or num_groups < 1 or S % (num_frames * num_groups)):
        raise RuntimeError(f"{what}: B'={S} is not a multiple of num_frames*num_groups={num_frames}*{num_groups}")
    return _out_shape(grad_layout, S, Q, C, P, num_frames, num_groups)


def _levels(feats, channels_first):
    """-> the C-ABI's level pointer array and [L, 2] (H, W) array of ``feats``"""
    hw_dims = slice(3, 5) if channels_first else slice(2, 4)
    ptrs = (ctypes.c_void_p * len(feats))(*[f.data_ptr() for f in feats])
    hw = (ctypes.c_int32 * (2 * len(feats)))(*[int(x) for f in feats for x in f.shape[hw_dims]])
    return ptrs, hw


def msmv_backward(grad_output, mlvl_feats, sampling_locations, scale_weights, grad_layout=_lib.OUT_SQCP, num_frames=1,
                  num_groups=1):
    """rac_msmv_bwd_ex: -> (grad_feats (list), grad_sampling_locations, grad_scale_weights), the tuple the
    reference's ``_ms_deform_attn_cuda_*_backward`` returns (msmv_sampling.cpp:302-497).  fp32 only.
    ``grad_layout=OUT_BQGTPC``: ``grad_output`` is ``[B, Q, G, T*P, C]`` (what msmv_forward writes with that layout), read as it
    lies; the results are those of the permuted [B', Q, C, P] gradient."""
    feats = list(mlvl_feats)
    L = len(feats)
    grad_output = grad_output.contiguous()
    _lib.require_gpu(grad_output, *feats, sampling_locations, scale_weights, what="msmv_sampling backward")
    if any(f.dtype != torch.float32 for f in feats):
        raise RuntimeError("msmv_sampling backward: float32 features only")
    S, N, C, Q, P = _shapes(feats, sampling_locations, scale_weights, False, "msmv_sampling backward")
    want = _grad_shape(grad_layout, S, Q, C, P, num_frames, num_groups, "msmv_sampling backward")
    if tuple(grad_output.shape) != want:
        raise RuntimeError(f"msmv_sampling backward: grad_output must be {list(want)}, got {list(grad_output.shape)}")
    grad_feats = [torch.zeros_like(f) for f in feats]
    grad_loc = torch.empty_like(sampling_locations)
    grad_w = torch.empty_like(scale_weights)
    ptrs, hw = _levels(feats, False)
    gptrs, _ = _levels(grad_feats, False)
    rc = _lib.lib().rac_msmv_bwd_ex(_lib.ptr(grad_output), grad_layout, num_frames, num_groups, ptrs, hw, L,
                                    _lib.ptr(sampling_locations), _lib.ptr(scale_weights), gptrs, _lib.ptr(grad_loc),
                                    _lib.ptr(grad_w), S, N, Q, P, C, _lib.stream_ptr())
    _lib.check(rc, "rac_msmv_bwd_ex")
    return grad_feats, grad_loc, grad_w


class _MSMVBase(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *args):
        *feats, sampling_locations, scale_weights = args
        ctx.save_for_backward(*feats, sampling_locations, scale_weights)
        return msmv_forward(feats, sampling_locations, scale_weights)

    @staticmethod
    def backward(ctx, grad_output):
        *feats, sampling_locations, scale_weights = ctx.saved_tensors
        grad_feats, grad_loc, grad_w = msmv_backward(grad_output, feats, sampling_locations, scale_weights)
        return (*grad_feats, grad_loc, grad_w)


class MSMVSamplingC2345(_MSMVBase):
    """wrapper.py:78-97 -- apply(feat_c2, feat_c3, feat_c4, feat_c5, sampling_locations, scale_weights)"""


class MSMVSamplingC45(_MSMVBase):
    """wrapper.py:99-118 -- apply(feat_c4, feat_c5, sampling_locations, scale_weights)"""


class MSMVSamplingC23456(_MSMVBase):
    """wrapper.py:120-142 -- apply(feat_c2, ..., feat_c6, sampling_locations, scale_weights)"""


def msmv_sampling(mlvl_feats, sampling_locations, scale_weights):
    """wrapper.py:145-153.  Any level count 1..8 is served by the HIP operator, forward and backward (the reference's
    other level counts take its differentiable torch path)."""
    if len(mlvl_feats) == 2:
        return MSMVSamplingC45.apply(*mlvl_feats, sampling_locations, scale_weights)
    if len(mlvl_feats) == 4:
        return MSMVSamplingC2345.apply(*mlvl_feats, sampling_locations, scale_weights)
    if len(mlvl_feats) == 5:
        return MSMVSamplingC23456.apply(*mlvl_feats, sampling_locations, scale_weights)
    return _MSMVBase.apply(*mlvl_feats, sampling_locations, scale_weights)


# ------------------------------------------------------------------------------------------ v2: hard level
def msmv_v2_forward(mlvl_feats, sampling_locations, scale_weights, out_layout=_lib.OUT_SQCP, num_frames=1, num_groups=1,
                    channels_first=False, out=None):
    """Launches rac_msmv_v2_fwd on the current stream: each point sampled on its argmax-weight level only, not scaled by
    the weight.  Features channel-last ``[B', N, H, W, C]`` (f32 / bf16) or, ``channels_first``, ``[B', C, N, H, W]``
    (f32).  ``out_layout=OUT_BQGTPC`` writes ``[B, Q, G, T*P, C]`` (what sampling_4d returns)."""
    feats = list(mlvl_feats)
    L = len(feats)
    _lib.require_gpu(*feats, sampling_locations, scale_weights, what="msmv_sampling_v2")
    S, N, C, Q, P = _shapes(feats, sampling_locations, scale_weights, channels_first, "msmv_sampling_v2")
    code = _lib.dtype_code(feats[0])
    if channels_first and code != _lib.RAC_F32:
        raise RuntimeError("msmv_sampling_v2: channel-first features must be float32")
    if out is None:
        out = torch.empty(_out_shape(out_layout, S, Q, C, P, num_frames, num_groups),
                          device=feats[0].device, dtype=torch.float32)
    ptrs, hw = _levels(feats, channels_first)
    rc = _lib.lib().rac_msmv_v2_fwd(ptrs, hw, L, _lib.ptr(sampling_locations), _lib.ptr(scale_weights), _lib.ptr(out),
                                    S, N, Q, P, C, code, _lib.FEAT_CF if channels_first else _lib.FEAT_CL, out_layout,
                                    num_frames, num_groups, _lib.stream_ptr())
    _lib.check(rc, "rac_msmv_v2_fwd")
    return out


def msmv_v2_backward(grad_output, mlvl_feats, sampling_locations, scale_weights, channels_first=False,
                     grad_layout=_lib.OUT_SQCP, num_frames=1, num_groups=1):
    """rac_msmv_v2_bwd_ex: -> (grad_feats (list, only the chosen levels' taps non-zero), grad_sampling_locations with a zero
    view component).  The weights get no gradient: argmax cuts the graph, as in the reference.  fp32 only.
    ``grad_layout`` / ``num_frames`` / ``num_groups``: as msmv_backward."""
    feats = list(mlvl_feats)
    L = len(feats)
    grad_output = grad_output.contiguous()
    _lib.require_gpu(grad_output, *feats, sampling_locations, scale_weights, what="msmv_sampling_v2 backward")
    if any(f.dtype != torch.float32 for f in feats):
        raise RuntimeError("msmv_sampling_v2 backward: float32 features only")
    S, N, C, Q, P = _shapes(feats, sampling_locations, scale_weights, channels_first, "msmv_sampling_v2 backward")
    want = _grad_shape(grad_layout, S, Q, C, P, num_frames, num_groups, "msmv_sampling_v2 backward")
    if tuple(grad_output.shape) != want:
        raise RuntimeError(f"msmv_sampling_v2 backward: grad_output must be {list(want)}, got {list(grad_output.shape)}")
    grad_feats = [torch.zeros_like(f) for f in feats]
    grad_loc = torch.empty_like(sampling_locations)
    ptrs, hw = _levels(feats, channels_first)
    gptrs, _ = _levels(grad_feats, channels_first)
    rc = _lib.lib().rac_msmv_v2_bwd_ex(_lib.ptr(grad_output), grad_layout, num_frames, num_groups, ptrs, hw, L,
                                       _lib.ptr(sampling_locations), _lib.ptr(scale_weights), gptrs, _lib.ptr(grad_loc), S, N,
                                       Q, P, C, _lib.FEAT_CF if channels_first else _lib.FEAT_CL, _lib.stream_ptr())
    _lib.check(rc, "rac_msmv_v2_bwd_ex")
    return grad_feats, grad_loc


class MSMVSamplingV2(torch.autograd.Function):
    """apply(channels_first, sampling_locations, scale_weights, *mlvl_feats) -> [B', Q, C, P]; gradients for the features
    and the locations, None for the weights."""

    @staticmethod
    def forward(ctx, channels_first, sampling_locations, scale_weights, *feats):
        ctx.channels_first = channels_first
        ctx.save_for_backward(sampling_locations, scale_weights, *feats)
        return msmv_v2_forward(feats, sampling_locations, scale_weights, channels_first=channels_first)

    @staticmethod
    def backward(ctx, grad_output):
        sampling_locations, scale_weights, *feats = ctx.saved_tensors
        grad_feats, grad_loc = msmv_v2_backward(grad_output, feats, sampling_locations, scale_weights,
                                                channels_first=ctx.channels_first)
        return (None, grad_loc, None, *grad_feats)


def msmv_sampling_v2(mlvl_feats, sampling_locations, scale_weights, channels_first=False):
    """wrapper.py:41-76 (msmv_sampling_v2): per point the level ``argmax(scale_weights)`` (torch.argmax rules) alone,
    bilinear, align_corners=True, zero padding, NOT multiplied by the weight -> ``[B', Q, C, P]`` float32.

    Features are channel-last ``[B', N, H, W, C]`` by default: that is what the decoder hands the op once ``MSMV_CUDA`` is
    true (it regroups the pyramid channel-last, racformer_transformer.py:116-118).  ``channels_first=True`` takes the
    ``[B', C, N, H, W]`` tensors of the reference's torch path (float32).  Same RuntimeErrors as ``msmv_sampling``; no CPU
    fallback.  Differentiable in the features and the locations (view component 0), not in the weights."""
    return MSMVSamplingV2.apply(bool(channels_first), sampling_locations, scale_weights, *mlvl_feats)
