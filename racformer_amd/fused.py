"""Python launchers of the two fully fused per-layer kernels (C-ABI: rac_sampling4d_fwd,
rac_bev_sampling_fwd).  The Linear outputs they consume may be column slices of one wide GEMM
output: only the last dimension has to be contiguous, the row stride is passed through."""
import ctypes
import functools

import torch

from . import _lib


@functools.lru_cache(maxsize=64)
def _depth_base(d_region, depth_num):
    """torch.linspace(-d_region, d_region, depth_num) as the reference evaluates it
    (racformer_transformer.py:395,515), computed once per (layer, depth_num) on the host."""
    vals = torch.linspace(-d_region, d_region, depth_num).tolist()
    return (ctypes.c_float * depth_num)(*vals)


def _rows(t, width, what):
    """[B,Q,width] view with unit last stride -> (pointer, row stride in floats)."""
    if not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError(f"racformer_amd.{what}: expected a float32 CUDA tensor")
    if t.shape[-1] != width or t.stride(-1) != 1 or (t.dim() == 3 and t.shape[0] > 1 and t.stride(0) != t.shape[1] * t.stride(1)):
        raise RuntimeError(f"racformer_amd.{what}: expected [B,Q,{width}] rows with unit inner stride")
    return _lib.ptr(t), int(t.stride(-2))


def _bev_rows(who, tensors, Hn, P, D, T, names=("offsets", "ray_logits", "scale_logits", "queue_logits")):
    """The four Linear outputs of a BEV stream (offsets, ray, scale, queue), or their gradients -> (pointers, row strides)."""
    rows = [_rows(t, width, f"{who}({name})") for t, width, name in zip(tensors, (Hn * P * 2, D, Hn * P, T), names)]
    return tuple(r[0] for r in rows), tuple(r[1] for r in rows)


def _dest(t, query_bbox, width):
    """A gradient destination [B,Q,width]: the caller's, or a new one."""
    if t is not None:
        return t
    return torch.empty(query_bbox.shape[:2] + (width,), device=query_bbox.device, dtype=torch.float32)


def _sized(who, name, t, numel, what):
    """An optional row-wise operand holds exactly the float32 elements its kernel reads (checked on any device, before a pointer
    is taken)."""
    if t is None:
        return
    if t.dtype != torch.float32 or t.numel() != numel:
        raise RuntimeError(f"{who}: {name} must hold {what} float32 elements, got {tuple(t.shape)} {t.dtype}")


def _row_operand(who, name, t, width=256):
    """A row operand of a row GEMM: [rows, width] or [B, Q, width] -> the rows it holds."""
    if t.dim() not in (2, 3) or t.shape[-1] != width:
        raise RuntimeError(f"{who}: {name} must be [rows, {width}] or [B, Q, {width}], got {tuple(t.shape)}")
    return int(torch.Size(t.shape[:-1]).numel())


def _pe_operands(who, linear, norm):
    """The position encoder's head as its kernels are built: Linear(3 -> 256), LayerNorm(256)."""
    if tuple(linear.weight.shape) != (256, 3) or linear.weight.dtype != torch.float32:
        raise RuntimeError(f"{who}: linear.weight must be float32 [256, 3], got {tuple(linear.weight.shape)}")
    _sized(who, "linear.bias", linear.bias, 256, "256")
    _sized(who, "norm.weight", norm.weight, 256, "256")
    _sized(who, "norm.bias", norm.bias, 256, "256")
    if linear.bias is None or norm.weight is None or norm.bias is None:
        raise RuntimeError(f"{who}: linear.bias, norm.weight and norm.bias are read by the kernel and must be present")


def _boxes_and_times(who, proposal, delta, time_diff_safe):
    """proposal, delta float32 [B,Q,10]; time_diff_safe float32 [B,T] (the kernels read entry [b, 1] where T > 1)."""
    if proposal.dim() != 3 or proposal.shape[-1] != 10 or proposal.dtype != torch.float32:
        raise RuntimeError(f"{who}: proposal must be float32 [B, Q, 10], got {tuple(proposal.shape)}")
    if tuple(delta.shape) != tuple(proposal.shape) or delta.dtype != torch.float32:
        raise RuntimeError(f"{who}: delta must be float32 and shaped like proposal {tuple(proposal.shape)}, got {tuple(delta.shape)}")
    if time_diff_safe.dim() != 2 or time_diff_safe.shape[0] != proposal.shape[0] or time_diff_safe.shape[1] < 1 \
            or time_diff_safe.dtype != torch.float32:
        raise RuntimeError(f"{who}: time_diff_safe must be float32 [B = {proposal.shape[0]}, T], got {tuple(time_diff_safe.shape)}")


def box_prep(query_bbox, pc_range):
    """[B,Q,10] polar boxes -> [B,Q,8] (cx,cy,cz,w,l,h,cos yaw,sin yaw), once per decoder layer."""
    _lib.require_gpu(query_bbox, what="box_prep")
    table = torch.empty(query_bbox.shape[:-1] + (8,), device=query_bbox.device, dtype=torch.float32)
    pc = (ctypes.c_float * 6)(*[float(v) for v in pc_range])
    rc = _lib.lib().rac_box_prep_fwd(_lib.ptr(query_bbox), _lib.ptr(table), query_bbox.numel() // 10, pc,
                                     _lib.stream_ptr())
    _lib.check(rc, "rac_box_prep_fwd")
    return table


_checked_views = set()


def sampling4d_fused(mlvl_feats, query_bbox, offsets, ray_logits, scale_logits, time_diff, lidar2img,
                     num_frames, num_groups, num_points, depth_num, pc_range, d_region, image_h, image_w,
                     eps=1e-5, debug=False, box_table=None, view_in=None, compact=None):
    """-> [B,Q,G,T*P,C] (and, with debug=True, the kernel's own locations [S,Q,P,3] and softmaxed scale
    weights [S,Q,P,L] for parity checks).  ``view_in`` (u8 [S,Q,P], parity tests only): camera index per point that
    replaces the kernel's own first-valid-view selection.  ``compact``: True / False selects the kernel variant that sets points
    without any tap aside (rigs that do not cover the full circle); None: by the number of cameras."""
    feats = list(mlvl_feats)
    L = len(feats)
    _lib.require_gpu(*feats, query_bbox, time_diff, lidar2img, what="sampling4d_fused")
    B, Q, _ = query_bbox.shape
    T, G, NP, D = num_frames, num_groups, num_points, depth_num
    P = NP * D
    S, N, _, _, C = feats[0].shape
    if S != B * T * G or lidar2img.shape[1] != T * N:
        raise RuntimeError("sampling4d_fused: feature slots / lidar2img do not match B*T*G / T*N")
    p_off, ld_off = _rows(offsets, G * P * 3, "sampling4d_fused(offsets)")
    p_ray, ld_ray = _rows(ray_logits, D, "sampling4d_fused(ray_logits)")
    p_sc, ld_sc = _rows(scale_logits, G * T * P * L, "sampling4d_fused(scale_logits)")
    if box_table is None:
        box_table = box_prep(query_bbox, pc_range)
    out = torch.empty(B, Q, G, T * P, C, device=query_bbox.device, dtype=torch.float32)
    loc_out = w_out = None
    capture = _lib.timer is not None and getattr(_lib.timer, "capture_inputs", False)
    want_debug, debug = debug, debug or capture
    if debug:
        loc_out = torch.empty(S, Q, P, 3, device=out.device, dtype=torch.float32)
        w_out = torch.empty(S, Q, P, L, device=out.device, dtype=torch.float32)
    if view_in is not None:
        if view_in.dtype != torch.uint8 or tuple(view_in.shape) != (S, Q, P) or not view_in.is_cuda or not view_in.is_contiguous():
            raise RuntimeError(f"sampling4d_fused: view_in must be a contiguous CUDA uint8 [{S},{Q},{P}] tensor")
        key = (view_in.data_ptr(), view_in._version, N)
        if key not in _checked_views:        # (a host read: once per tensor, so that a captured plan's forwards issue none)
            if int(view_in.max()) >= N:
                raise RuntimeError("sampling4d_fused: view_in holds a camera index >= N")
            if len(_checked_views) > 256:
                _checked_views.clear()
            _checked_views.add(key)
    ptrs = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats])
    hw = (ctypes.c_int32 * (2 * L))(*[int(x) for f in feats for x in f.shape[2:4]])
    pc = (ctypes.c_float * 6)(*[float(v) for v in pc_range])
    ev = _lib.timer.record("sampling4d_fwd") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    rc = _lib.lib().rac_sampling4d_fwd(
        ptrs, hw, L, _lib.ptr(query_bbox), _lib.ptr(box_table), p_off, p_ray, p_sc, _lib.ptr(time_diff), _lib.ptr(lidar2img),
        _lib.ptr(out), _lib.ptr(loc_out) if debug else None, _lib.ptr(w_out) if debug else None,
        _lib.ptr(view_in) if view_in is not None else None, ld_off, ld_ray, ld_sc, B, T, N, G, Q, NP, D, C, pc, _depth_base(float(d_region), D), float(d_region),
        float(image_h), float(image_w), float(eps), _lib.dtype_code(feats[0]), -1 if compact is None else int(bool(compact)), _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_sampling4d_fwd")
    if capture:  # bench.py: the locations this launch sampled at, for the algorithmic-byte count
        _lib.timer.captured.append((loc_out, [tuple(f.shape) for f in feats]))
    return (out, loc_out, w_out) if want_debug else out


def sampling4d_backward(mlvl_feats, query_bbox, offsets, ray_logits, scale_logits, time_diff, lidar2img, grad_out,
                        num_frames, num_groups, num_points, depth_num, pc_range, d_region, image_h, image_w, eps=1e-5,
                        box_table=None, view_in=None, grad_offsets=None, grad_ray=None, grad_scale=None, want_feats=True,
                        debug=False):
    """Backward of sampling4d_fused (rac_sampling4d_bwd): the forward's arguments and grad_out [B,Q,G,T*P,64] ->
    (grad_feats (a list shaped as mlvl_feats; None with ``want_feats=False``: the scatter is skipped), grad_offsets, grad_ray,
    grad_scale (of the logits), grad_box [B,Q,8]); with ``debug`` also the kernel's per-keypoint gradients and its recomputed
    keypoints (grad_loc [S,Q,P,2], grad_w [S,Q,P,L], loc [S,Q,P,3], w [S,Q,P,L]).  ``grad_offsets`` .. ``grad_scale``:
    destinations with unit inner stride and a row stride of their own (column slices of one gradient of a fused Linear
    output); allocated when not given.  Every element of them is written.  ``view_in``: what the forward was given.
    float32 features only."""
    feats = list(mlvl_feats)
    L = len(feats)
    _lib.require_gpu(*feats, query_bbox, time_diff, lidar2img, grad_out, what="sampling4d_backward")
    if any(f.dtype != torch.float32 for f in feats):
        raise RuntimeError("sampling4d_backward: float32 features only")
    B, Q, _ = query_bbox.shape
    T, G, NP, D = num_frames, num_groups, num_points, depth_num
    P = NP * D
    S, N, _, _, C = feats[0].shape
    if S != B * T * G or lidar2img.shape[1] != T * N:
        raise RuntimeError("sampling4d_backward: feature slots / lidar2img do not match B*T*G / T*N")
    if tuple(grad_out.shape) != (B, Q, G, T * P, C) or grad_out.dtype != torch.float32 or not grad_out.is_contiguous():
        raise RuntimeError(f"sampling4d_backward: grad_out must be a contiguous float32 [{B},{Q},{G},{T * P},{C}]")
    p_off, ld_off = _rows(offsets, G * P * 3, "sampling4d_backward(offsets)")
    p_ray, ld_ray = _rows(ray_logits, D, "sampling4d_backward(ray_logits)")
    p_sc, ld_sc = _rows(scale_logits, G * T * P * L, "sampling4d_backward(scale_logits)")
    if box_table is None:
        box_table = box_prep(query_bbox, pc_range)
    if view_in is not None and (view_in.dtype != torch.uint8 or tuple(view_in.shape) != (S, Q, P) or not view_in.is_cuda
                                or not view_in.is_contiguous()):
        raise RuntimeError(f"sampling4d_backward: view_in must be a contiguous CUDA uint8 [{S},{Q},{P}] tensor")
    dev = query_bbox.device
    grad_offsets, grad_ray = _dest(grad_offsets, query_bbox, G * P * 3), _dest(grad_ray, query_bbox, D)
    grad_scale = _dest(grad_scale, query_bbox, G * T * P * L)
    p_goff, gld_off = _rows(grad_offsets, G * P * 3, "sampling4d_backward(grad_offsets)")
    p_gray, gld_ray = _rows(grad_ray, D, "sampling4d_backward(grad_ray)")
    p_gsc, gld_sc = _rows(grad_scale, G * T * P * L, "sampling4d_backward(grad_scale)")
    grad_feats = [torch.zeros_like(f) for f in feats] if want_feats else None
    grad_box = torch.empty(B, Q, 8, device=dev, dtype=torch.float32)
    grad_loc = grad_w = loc = w = None
    if debug:
        grad_loc = torch.empty(S, Q, P, 2, device=dev, dtype=torch.float32)
        grad_w = torch.empty(S, Q, P, L, device=dev, dtype=torch.float32)
        loc = torch.empty(S, Q, P, 3, device=dev, dtype=torch.float32)
        w = torch.empty(S, Q, P, L, device=dev, dtype=torch.float32)
    ptrs = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats])
    gptrs = (ctypes.c_void_p * L)(*[f.data_ptr() for f in grad_feats]) if want_feats else None
    hw = (ctypes.c_int32 * (2 * L))(*[int(x) for f in feats for x in f.shape[2:4]])
    pc = (ctypes.c_float * 6)(*[float(v) for v in pc_range])
    ev = _lib.timer.record("sampling4d_bwd") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    rc = _lib.lib().rac_sampling4d_bwd(
        ptrs, hw, L, _lib.ptr(query_bbox), _lib.ptr(box_table), p_off, p_ray, p_sc, _lib.ptr(time_diff), _lib.ptr(lidar2img),
        _lib.ptr(view_in) if view_in is not None else None, _lib.ptr(grad_out), gptrs, p_goff, p_gray, p_gsc, _lib.ptr(grad_box),
        _lib.ptr(grad_loc) if debug else None, _lib.ptr(grad_w) if debug else None, _lib.ptr(loc) if debug else None,
        _lib.ptr(w) if debug else None, ld_off, ld_ray, ld_sc, gld_off, gld_ray, gld_sc, B, T, N, G, Q, NP, D, C, pc,
        _depth_base(float(d_region), D), float(d_region), float(image_h), float(image_w), float(eps), _lib.RAC_F32, _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_sampling4d_bwd")
    res = (grad_feats, grad_offsets, grad_ray, grad_scale, grad_box)
    return res + (grad_loc, grad_w, loc, w) if debug else res


def bev_sampling_fused(value, hw, query_bbox, offsets, ray_logits, scale_logits, queue_logits, time_diff,
                       num_frames, num_heads, num_points, depth_num, pc_range, d_region, debug=False, box_table=None,
                       out=None):
    """value [B*T, H*W, heads, 64] -> [B,Q,heads*64] (frame-fused, before output_proj)."""
    _lib.require_gpu(value, query_bbox, time_diff, what="bev_sampling_fused")
    B, Q, _ = query_bbox.shape
    T, Hn, NP, D = num_frames, num_heads, num_points, depth_num
    P = NP * D
    H, W = hw
    if tuple(value.shape) != (B * T, H * W, Hn, 64):
        raise RuntimeError(f"bev_sampling_fused: value must be [{B * T},{H * W},{Hn},64], got {tuple(value.shape)}")
    ptrs, lds = _bev_rows("bev_sampling_fused", (offsets, ray_logits, scale_logits, queue_logits), Hn, P, D, T)
    if box_table is None:
        box_table = box_prep(query_bbox, pc_range)
    if out is None:
        out = torch.empty(B, Q, Hn * 64, device=query_bbox.device, dtype=torch.float32)
    elif not out.is_contiguous() or tuple(out.shape) != (B, Q, Hn * 64):
        raise RuntimeError("bev_sampling_fused: out must be a contiguous [B,Q,heads*64] tensor")
    loc_out = torch.empty(B, Q, Hn, T, P, 2, device=out.device, dtype=torch.float32) if debug else None
    pc = (ctypes.c_float * 6)(*[float(v) for v in pc_range])
    ev = _lib.timer.record("bev_sampling_fwd") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    rc = _lib.lib().rac_bev_sampling_fwd(
        _lib.ptr(value), _lib.ptr(query_bbox), _lib.ptr(box_table), *ptrs, _lib.ptr(time_diff), _lib.ptr(out),
        _lib.ptr(loc_out) if debug else None, *lds, B, T, Q, Hn, NP, D, H, W, 64, pc,
        _depth_base(float(d_region), D), float(d_region), _lib.dtype_code(value), _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_bev_sampling_fwd")
    return (out, loc_out) if debug else out


BEV_BWD_LDS_LIMIT = 160 * 1024


def bev_backward_batch_fits(B, num_heads, num_frames, points):
    """Whether rac_bev_sampling_bwd_batch accepts a batch of B: its workgroup stages a query index of all B samples in LDS
    (bev_bwd_lds_floats in bev_fused_bwd.hip; tests/test_bev_sampling_batch_grad_cpu.py holds the two together)."""
    per_sample = num_heads * num_frames * points * 6 + num_heads * points * 8 + num_heads * 64 + num_frames * 3 + 16 * 2 + 16
    return B >= 1 and num_frames <= 64 and points <= 64 and 4 * B * per_sample <= BEV_BWD_LDS_LIMIT


def bev_sampling_backward(value, hw, query_bbox, offsets, ray_logits, scale_logits, queue_logits, time_diff, grad_out,
                          num_frames, num_heads, num_points, depth_num, pc_range, d_region, box_table=None, grad_offsets=None,
                          grad_ray=None, grad_scale=None, grad_queue=None, debug=False, batch_symbol=None):
    """Backward of bev_sampling_fused (rac_bev_sampling_bwd at B == 1, rac_bev_sampling_bwd_batch at B > 1, which reproduces the
    forward's frame / batch pairing): the forward's arguments and grad_out [B,Q,heads*64] ->
    (grad_value [B*T,H*W,heads,64], grad_offsets, grad_ray, grad_scale, grad_queue, grad_box [B,Q,8]); with ``debug`` also
    the kernel's per-keypoint gradients (grad_loc [B,Q,heads,T,P,2], grad_attn [B,Q,heads,T,P]).  ``grad_offsets`` ..
    ``grad_queue``: destinations with unit inner stride and a row stride of their own (column slices of one gradient of a
    fused Linear output); allocated when not given.  Every element of them is written.  float32 values only; a batch whose
    keypoints exceed a workgroup's LDS is refused (RuntimeError).  ``batch_symbol``: True / False picks the entry point whatever
    B is (the tests compare the two at B == 1)."""
    _lib.require_gpu(value, query_bbox, time_diff, grad_out, what="bev_sampling_backward")
    B, Q, _ = query_bbox.shape
    T, Hn, NP, D = num_frames, num_heads, num_points, depth_num
    P = NP * D
    H, W = hw
    if tuple(value.shape) != (B * T, H * W, Hn, 64):
        raise RuntimeError(f"bev_sampling_backward: value must be [{B * T},{H * W},{Hn},64], got {tuple(value.shape)}")
    if tuple(grad_out.shape) != (B, Q, Hn * 64) or grad_out.dtype != torch.float32 or not grad_out.is_contiguous():
        raise RuntimeError(f"bev_sampling_backward: grad_out must be a contiguous float32 [{B},{Q},{Hn * 64}]")
    ptrs, lds = _bev_rows("bev_sampling_backward", (offsets, ray_logits, scale_logits, queue_logits), Hn, P, D, T)
    if box_table is None:
        box_table = box_prep(query_bbox, pc_range)
    dev = query_bbox.device
    grad_offsets, grad_ray = _dest(grad_offsets, query_bbox, Hn * P * 2), _dest(grad_ray, query_bbox, D)
    grad_scale, grad_queue = _dest(grad_scale, query_bbox, Hn * P), _dest(grad_queue, query_bbox, T)
    gptrs, glds = _bev_rows("bev_sampling_backward", (grad_offsets, grad_ray, grad_scale, grad_queue), Hn, P, D, T,
                            names=("grad_offsets", "grad_ray", "grad_scale", "grad_queue"))
    grad_value = torch.zeros(value.shape, device=dev, dtype=torch.float32)
    grad_box = torch.empty(B, Q, 8, device=dev, dtype=torch.float32)
    grad_loc = torch.empty(B, Q, Hn, T, P, 2, device=dev, dtype=torch.float32) if debug else None
    grad_attn = torch.empty(B, Q, Hn, T, P, device=dev, dtype=torch.float32) if debug else None
    pc = (ctypes.c_float * 6)(*[float(v) for v in pc_range])
    code = _lib.dtype_code(value) if value.dtype in (torch.float32, torch.bfloat16) else _lib.RAC_I16
    ev = _lib.timer.record("bev_sampling_bwd") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    symbol = "rac_bev_sampling_bwd_batch" if (B != 1 if batch_symbol is None else batch_symbol) else "rac_bev_sampling_bwd"
    rc = getattr(_lib.lib(), symbol)(
        _lib.ptr(value), _lib.ptr(query_bbox), _lib.ptr(box_table), *ptrs, _lib.ptr(time_diff),
        _lib.ptr(grad_out), _lib.ptr(grad_value), *gptrs, _lib.ptr(grad_box),
        _lib.ptr(grad_loc) if debug else None, _lib.ptr(grad_attn) if debug else None, *lds, *glds,
        B, T, Q, Hn, NP, D, H, W, 64, pc, _depth_base(float(d_region), D), float(d_region), code, _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, symbol)
    res = (grad_value, grad_offsets, grad_ray, grad_scale, grad_queue, grad_box)
    return res + (grad_loc, grad_attn) if debug else res


def quantize_values_i16(value):
    """A hoisted value stream [B*T, H*W, heads, 64] f32 -> (int16 mantissas of the same shape, scales [B*T, H*W, heads] f32):
    one power-of-two scale per (pixel, head) block of 64 channels, value = q * scale (rac_quant_i16_fwd; opt-in storage of
    RaCFormerTransformerDecoderLayer.value_storage = "i16")."""
    _lib.require_gpu(value, what="quantize_values_i16")
    if value.dtype != torch.float32 or value.shape[-1] != 64:
        raise RuntimeError("quantize_values_i16: float32 [..., 64] value stream expected")
    q = torch.empty(value.shape, device=value.device, dtype=torch.int16)
    scale = torch.empty(value.shape[:-1], device=value.device, dtype=torch.float32)
    ev = _lib.timer.record("quant_i16_fwd") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    rc = _lib.lib().rac_quant_i16_fwd(_lib.ptr(value), _lib.ptr(q), _lib.ptr(scale), scale.numel(), _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_quant_i16_fwd")
    return q, scale


def bev_sampling_multi_fused(streams, hw, query_bbox, time_diff, num_frames, num_heads, num_points, depth_num, pc_range,
                             d_region, box_table, out, value_scales=None):
    """The BEV streams of one decoder layer in one launch (rac_bev_sampling_multi_fwd).  ``streams``: list of
    (value [B*T,H*W,heads,64], offsets, ray_logits, scale_logits, queue_logits) with equal row strides; ``out`` [n,B,Q,heads*64].
    ``value_scales``: per stream the [B*T,H*W,heads] scale table of an int16 block-stored value stream (quantize_values_i16;
    rac_bev_sampling_multi_q16_fwd)."""
    B, Q, _ = query_bbox.shape
    T, Hn, NP, D = num_frames, num_heads, num_points, depth_num
    P = NP * D
    H, W = hw
    n = len(streams)
    if tuple(out.shape) != (n, B, Q, Hn * 64) or not out.is_contiguous():
        raise RuntimeError("bev_sampling_multi_fused: out must be a contiguous [streams,B,Q,heads*64] tensor")
    lds = None
    cols = [[], [], [], [], []]
    for value, off, ray, sc, qu in streams:
        _lib.require_gpu(value, what="bev_sampling_multi_fused")
        if tuple(value.shape) != (B * T, H * W, Hn, 64):
            raise RuntimeError(f"bev_sampling_multi_fused: value must be [{B * T},{H * W},{Hn},64], got {tuple(value.shape)}")
        ptrs, ld = _bev_rows("bev_sampling_multi_fused", (off, ray, sc, qu), Hn, P, D, T)
        if lds is None:
            lds = ld
        elif lds != ld or value.dtype != streams[0][0].dtype:
            raise RuntimeError("bev_sampling_multi_fused: the streams must share row strides and dtype")
        for c, v in zip(cols, (value.data_ptr(),) + tuple(x.value for x in ptrs)):
            c.append(v)
    arr = [(ctypes.c_void_p * n)(*c) for c in cols]
    outs = (ctypes.c_void_p * n)(*[out[i].data_ptr() for i in range(n)])
    pc = (ctypes.c_float * 6)(*[float(v) for v in pc_range])
    ev = _lib.timer.record(f"bev_sampling_x{n}_fwd") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    if value_scales is not None:
        if len(value_scales) != n or any(v[0].dtype != torch.int16 for v in streams):
            raise RuntimeError("bev_sampling_multi_fused: int16 value streams and one scale table per stream expected")
        for sc_ in value_scales:
            _lib.require_gpu(sc_, what="bev_sampling_multi_fused(value_scales)")
            if tuple(sc_.shape) != (B * T, H * W, Hn) or sc_.dtype != torch.float32:
                raise RuntimeError(f"bev_sampling_multi_fused: scale table must be f32 [{B * T},{H * W},{Hn}]")
        vsc = (ctypes.c_void_p * n)(*[sc_.data_ptr() for sc_ in value_scales])
        rc = _lib.lib().rac_bev_sampling_multi_q16_fwd(
            n, arr[0], vsc, arr[1], arr[2], arr[3], arr[4], outs, _lib.ptr(query_bbox), _lib.ptr(box_table), _lib.ptr(time_diff),
            *lds, B, T, Q, Hn, NP, D, H, W, 64, pc, _depth_base(float(d_region), D), float(d_region),
            _lib.stream_ptr())
    else:
        rc = _lib.lib().rac_bev_sampling_multi_fwd(
            n, arr[0], arr[1], arr[2], arr[3], arr[4], outs, _lib.ptr(query_bbox), _lib.ptr(box_table), _lib.ptr(time_diff),
            *lds, B, T, Q, Hn, NP, D, H, W, 64, pc, _depth_base(float(d_region), D), float(d_region),
            _lib.dtype_code(streams[0][0]), _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_bev_sampling_multi_fwd")
    return out


class PackedAttnMask:
    """A boolean [Q,Q] attention mask (True: query i does not attend to key j) in the two forms its users read: ``bits``, the
    int32 view [Q, ceil(Q/32)] of the uint32 words rac_sasa_fwd_mask / rac_sasa_bwd_mask take (bit j & 31 of word [i][j >> 5]),
    and ``dense``, the bool tensor itself (forward_unfused).  Built by pack_attn_mask."""

    __slots__ = ("bits", "dense")

    def __init__(self, bits, dense):
        self.bits, self.dense = bits, dense


def pack_attn_mask(mask_bool):
    """bool [Q,Q] -> PackedAttnMask.  torch ops on the mask's device only: no host synchronisation."""
    if isinstance(mask_bool, PackedAttnMask):
        return mask_bool
    if mask_bool.dim() != 2 or mask_bool.shape[0] != mask_bool.shape[1] or mask_bool.dtype != torch.bool:
        raise RuntimeError(f"pack_attn_mask: expected a bool [Q,Q] mask, got {mask_bool.dtype} {list(mask_bool.shape)}")
    Q = mask_bool.shape[0]
    W = (Q + 31) // 32
    m = torch.nn.functional.pad(mask_bool, (0, W * 32 - Q)).view(Q, W, 32).to(torch.int64)
    words = (m << torch.arange(32, device=mask_bool.device, dtype=torch.int64)).sum(-1)      # 0 .. 2^32 - 1
    words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)             # the same 32 bits, as int32
    return PackedAttnMask(words.contiguous(), mask_bool)


def _mask_words(mask, Q, what):
    """(pointer, ld_mask) of a PackedAttnMask's words for a [.,Q,.] problem"""
    if not isinstance(mask, PackedAttnMask):
        raise RuntimeError(f"{what}: mask must be a PackedAttnMask (pack_attn_mask)")
    bits = mask.bits
    _lib.require_gpu(bits, what=f"{what}(mask)")
    if bits.dtype != torch.int32 or bits.dim() != 2 or bits.shape[0] != Q or bits.shape[1] < (Q + 31) // 32 or not bits.is_contiguous():
        raise RuntimeError(f"{what}: mask words must be contiguous int32 [{Q}, >= {(Q + 31) // 32}], got {list(bits.shape)}")
    return _lib.ptr(bits), bits.shape[1]


def sasa_fused(qkv, tau, query_bbox, num_heads, pc_range, box_table=None, lse_out=None, mask=None):
    """qkv [B,Q,3*E] (q|k|v, each [heads, E/heads]; may be a column slice), tau [B,Q,heads] ->
    attention output [B,Q,E] before out_proj.
    ``lse_out``: optional contiguous f32 [B,heads,Q] that receives every query row's log-sum-exp (rac_sasa_fwd_ex, for
    sasa_backward); the output is bit-identical either way.
    ``mask``: optional PackedAttnMask shared by all batches and heads (rac_sasa_fwd_mask): blocked pairs get probability 0."""
    _lib.require_gpu(query_bbox, what="sasa_fused")
    B, Q, _ = query_bbox.shape
    E = qkv.shape[-1] // 3
    p_qkv, ld_qkv = _rows(qkv, 3 * E, "sasa_fused(qkv)")
    p_tau, ld_tau = _rows(tau, num_heads, "sasa_fused(tau)")
    if lse_out is not None:
        _lib.require_gpu(lse_out, what="sasa_fused(lse_out)")
        if tuple(lse_out.shape) != (B, num_heads, Q) or lse_out.dtype != torch.float32:
            raise RuntimeError(f"sasa_fused: lse_out must be float32 [{B},{num_heads},{Q}]")
    out = torch.empty(B, Q, E, device=qkv.device, dtype=torch.float32)
    pc = (ctypes.c_float * 6)(*[float(v) for v in pc_range])
    ev = _lib.timer.record("sasa_fwd") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    box = _lib.ptr(box_table) if box_table is not None else None
    if mask is not None:
        p_mask, ld_mask = _mask_words(mask, Q, "sasa_fused")
        rc = _lib.lib().rac_sasa_fwd_mask(p_qkv, p_tau, _lib.ptr(query_bbox), box, _lib.ptr(out),
                                          _lib.ptr(lse_out) if lse_out is not None else None, ld_qkv, ld_tau, B, Q, num_heads,
                                          E // num_heads, pc, _lib.stream_ptr(), p_mask, ld_mask)
    elif lse_out is None:
        rc = _lib.lib().rac_sasa_fwd(p_qkv, p_tau, _lib.ptr(query_bbox), box, _lib.ptr(out), ld_qkv, ld_tau, B, Q, num_heads,
                                     E // num_heads, pc, _lib.stream_ptr())
    else:
        rc = _lib.lib().rac_sasa_fwd_ex(p_qkv, p_tau, _lib.ptr(query_bbox), box, _lib.ptr(out), _lib.ptr(lse_out), ld_qkv,
                                        ld_tau, B, Q, num_heads, E // num_heads, pc, _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_sasa_fwd_mask" if mask is not None else "rac_sasa_fwd" if lse_out is None else "rac_sasa_fwd_ex")
    return out


def sasa_backward(qkv, tau, query_bbox, num_heads, pc_range, out, lse, grad_out, box_table=None, grad_qkv=None, grad_tau=None,
                  mask=None):
    """Backward of sasa_fused (rac_sasa_bwd; rac_sasa_bwd_mask with ``mask``): qkv, tau, query_bbox, box_table, mask as given to
    it, out and lse what it returned and
    wrote, grad_out [B,Q,E] -> (grad_qkv [B,Q,3*E], grad_tau [B,Q,heads]).  ``grad_qkv`` / ``grad_tau``: destinations with
    unit inner stride and a row stride of their own (e.g. the two column slices of one [B,Q,3*E+heads] buffer); allocated as
    that one buffer when not given.  Every element of both is written."""
    _lib.require_gpu(query_bbox, out, lse, grad_out, what="sasa_backward")
    B, Q, _ = query_bbox.shape
    E = qkv.shape[-1] // 3
    p_qkv, ld_qkv = _rows(qkv, 3 * E, "sasa_backward(qkv)")
    p_tau, ld_tau = _rows(tau, num_heads, "sasa_backward(tau)")
    for t_, shape, what in ((out, (B, Q, E), "out"), (grad_out, (B, Q, E), "grad_out"), (lse, (B, num_heads, Q), "lse")):
        if tuple(t_.shape) != shape or t_.dtype != torch.float32:
            raise RuntimeError(f"sasa_backward: {what} must be float32 {list(shape)}")
    if grad_qkv is None or grad_tau is None:
        wide = torch.empty(B, Q, 3 * E + num_heads, device=qkv.device, dtype=torch.float32)
        grad_qkv, grad_tau = wide[..., :3 * E], wide[..., 3 * E:]
    p_gqkv, ld_gqkv = _rows(grad_qkv, 3 * E, "sasa_backward(grad_qkv)")
    p_gtau, ld_gtau = _rows(grad_tau, num_heads, "sasa_backward(grad_tau)")
    pc = (ctypes.c_float * 6)(*[float(v) for v in pc_range])
    ev = _lib.timer.record("sasa_bwd") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    args = (p_qkv, p_tau, _lib.ptr(query_bbox), _lib.ptr(box_table) if box_table is not None else None,
            _lib.ptr(out), _lib.ptr(lse), _lib.ptr(grad_out), p_gqkv, p_gtau, ld_qkv, ld_tau, ld_gqkv,
            ld_gtau, B, Q, num_heads, E // num_heads, pc, _lib.stream_ptr())
    if mask is not None:
        rc = _lib.lib().rac_sasa_bwd_mask(*args, *_mask_words(mask, Q, "sasa_backward"))
    else:
        rc = _lib.lib().rac_sasa_bwd(*args)
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_sasa_bwd_mask" if mask is not None else "rac_sasa_bwd")
    return grad_qkv, grad_tau


def mixing_fused(x, params, in_points, n_groups, out_points=128, eps=1e-5, split=False, param_scale=1.0, f16x3=False, out=None,
                 period=None):
    """x [B,Q,G,P,64] (contiguous), params [B,Q,G*(64*64+128*P)] (unit inner stride) ->
    relu(LN(S @ relu(LN(x @ M)))) as [B,Q,G*128*64], ready for out_proj.
    ``split=True``: instead returns the f16 line image [B*Q, G*256, hi 32 | lo 32] of the same values * SPLIT_ACT_SCALE
    (A operand of rac_outproj_fwd: every value stored once as hi + lo).
    ``param_scale``: factor applied to every parameter on load (the power-of-two alpha of a split generator GEMM).
    ``f16x3``: run the two products as 3-product split-precision f16 MFMAs (RAC_MIX_F16X3) instead of f32-input MFMAs.
    ``out``: write into this tensor (a row range of a larger image) instead of allocating.
    ``period``: params holds ``period`` rows (a divisor of B*Q) and item row r reads row r % period (rac_mixing_period_fwd):
    the parameters of batch elements generated from the same queries, held once."""
    _lib.require_gpu(x, what="mixing_fused")
    B, Q, G, P, C = x.shape
    if G != n_groups or P != in_points or x.dtype != torch.float32:
        raise RuntimeError("mixing_fused: x must be float32 [B,Q,G,P,64]")
    width = G * (C * C + out_points * P)
    p_par, ld_par = _rows(params, width, "mixing_fused(params)")
    rows = params.numel() // params.shape[-1]
    if period is None:
        period = B * Q
    if period < 1 or (B * Q) % period != 0 or rows != period or params.dtype != torch.float32:
        raise RuntimeError(f"mixing_fused: params must be float32 with {period} rows (a divisor of {B * Q}), got {rows}")
    if out is not None:
        want = ((B * Q, G * out_points * C // 32, 64), torch.float16) if split else ((B, Q, G * out_points * C), torch.float32)
        if tuple(out.shape) != want[0] or out.dtype != want[1] or not out.is_contiguous() or not out.is_cuda:
            raise RuntimeError(f"mixing_fused: out must be a contiguous CUDA {want[1]} tensor of shape {want[0]}")
    elif split:
        out = torch.empty(B * Q, G * out_points * C // 32, 64, device=x.device, dtype=torch.float16)
    else:
        out = torch.empty(B, Q, G * out_points * C, device=x.device, dtype=torch.float32)
    ev = _lib.timer.record("mixing_fwd") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    head = (_lib.ptr(x), p_par, float(param_scale), None if split else _lib.ptr(out), _lib.ptr(out) if split else None,
            SPLIT_ACT_SCALE, ld_par)
    tail = (B * Q, G, P, C, out_points, float(eps), _lib.MIX_F16X3 if f16x3 else _lib.MIX_F32, _lib.stream_ptr())
    if period != B * Q:
        rc = _lib.lib().rac_mixing_period_fwd(*head, int(period), *tail)
    else:
        rc = _lib.lib().rac_mixing_fwd(*head, *tail)
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_mixing_fwd")
    return out


def mixing_backward(x, params, grad_out, in_points, n_groups, out_points=128, eps=1e-5, grad_x=None, grad_params=None, z_out=None):
    """Backward of mixing_fused(..., f16x3=False, param_scale=1) (rac_mixing_bwd): x [B,Q,G,P,64] (contiguous) and params
    [B,Q,G*(64*64+128*P)] (unit inner stride) as given to it, grad_out [B,Q,G*128*64] -> (grad_x [B,Q,G,P,64],
    grad_params [B,Q,G*(64*64+128*P)]).  ``grad_x`` / ``grad_params``: destinations (grad_params may have a row stride of its
    own); allocated when not given.  Every element of both is written.  ``z_out``: optional contiguous f32 [B,Q,G*128*64]
    receiving the recomputed forward output."""
    _lib.require_gpu(x, grad_out, what="mixing_backward")
    B, Q, G, P, C = x.shape
    if G != n_groups or P != in_points or x.dtype != torch.float32 or not x.is_contiguous():
        raise RuntimeError("mixing_backward: x must be contiguous float32 [B,Q,G,P,64]")
    width = G * (C * C + out_points * P)
    p_par, ld_par = _rows(params, width, "mixing_backward(params)")
    want = (B, Q, G * out_points * C)
    if tuple(grad_out.shape) != want or grad_out.dtype != torch.float32 or not grad_out.is_contiguous():
        raise RuntimeError(f"mixing_backward: grad_out must be contiguous float32 {list(want)}")
    if z_out is not None:
        _lib.require_gpu(z_out, what="mixing_backward(z_out)")
        if tuple(z_out.shape) != want or z_out.dtype != torch.float32 or not z_out.is_contiguous():
            raise RuntimeError(f"mixing_backward: z_out must be contiguous float32 {list(want)}")
    if grad_x is None:
        grad_x = torch.empty_like(x)
    elif tuple(grad_x.shape) != tuple(x.shape) or grad_x.dtype != torch.float32 or not grad_x.is_contiguous() or not grad_x.is_cuda:
        raise RuntimeError("mixing_backward: grad_x must be a contiguous CUDA float32 tensor shaped like x")
    if grad_params is None:
        grad_params = torch.empty(B, Q, width, device=x.device, dtype=torch.float32)
    p_gpar, ld_gpar = _rows(grad_params, width, "mixing_backward(grad_params)")
    ev = _lib.timer.record("mixing_bwd") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    rc = _lib.lib().rac_mixing_bwd(_lib.ptr(x), p_par, ld_par, _lib.ptr(grad_out), _lib.ptr(grad_x), p_gpar, ld_gpar,
                                   _lib.ptr(z_out) if z_out is not None else None, B * Q, G, P, C, out_points, float(eps),
                                   _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_mixing_bwd")
    return grad_x, grad_params


def refine_fused(proposal, delta, time_diff_safe, num_ray):
    """refine_bbox + velocity / time_diff + theta_d2xy in one launch.
    -> (bbox_pred [B,Q,10] polar, bbox_xy [B,Q,10] normalised xy)."""
    _boxes_and_times("refine_fused", proposal, delta, time_diff_safe)
    proposal, delta = proposal.contiguous(), delta.contiguous()
    _lib.require_gpu(proposal, delta, time_diff_safe, what="refine_fused")
    B, Q, _ = proposal.shape
    pred, xy = torch.empty_like(proposal), torch.empty_like(proposal)
    rc = _lib.lib().rac_refine_fwd(_lib.ptr(proposal), _lib.ptr(delta), _lib.ptr(time_diff_safe), _lib.ptr(pred),
                                   _lib.ptr(xy), B, Q, time_diff_safe.shape[1], float(num_ray), _lib.stream_ptr())
    _lib.check(rc, "rac_refine_fwd")
    return pred, xy


def refine_backward(proposal, delta, time_diff_safe, num_ray, grad_pred=None, grad_xy=None):
    """Backward of refine_fused in one launch (rac_refine_bwd): (grad_pred, grad_xy) [B,Q,10] each, either may be None (absent: not
    allocated, not read) -> (grad_delta, grad_proposal) [B,Q,10]."""
    proposal, delta = proposal.contiguous(), delta.contiguous()
    grad_pred, grad_xy = (g.contiguous() if g is not None else None for g in (grad_pred, grad_xy))
    grads = [g for g in (grad_pred, grad_xy) if g is not None]
    _lib.require_gpu(proposal, delta, time_diff_safe, *grads, what="refine_backward")
    for g in grads:
        if g.dtype != torch.float32 or tuple(g.shape) != tuple(proposal.shape):
            raise RuntimeError("refine_backward: gradients must be float32 tensors shaped like the boxes")
    B, Q, _ = proposal.shape
    grad_delta, grad_proposal = torch.empty_like(delta), torch.empty_like(proposal)
    gp = _lib.ptr(grad_pred) if grad_pred is not None else None
    gx = _lib.ptr(grad_xy) if grad_xy is not None else None
    rc = _lib.lib().rac_refine_bwd(_lib.ptr(proposal), _lib.ptr(delta), _lib.ptr(time_diff_safe), gp, gx, _lib.ptr(grad_delta),
                                   _lib.ptr(grad_proposal), B, Q, time_diff_safe.shape[1], float(num_ray), _lib.stream_ptr())
    _lib.check(rc, "rac_refine_bwd")
    return grad_delta, grad_proposal


def regroup_fused(feats, dims, groups, out_dtype=torch.float32):
    """feats[l] contiguous float32 [B,T*N,G*C,H,W] -> [B*T*G,N,H,W,C] of ``out_dtype``, dims = (B, T, N, C): ONE launch over all
    levels (rac_regroup_multi_fwd); levels whose sizes are not multiples of 4 go through the scalar per-level kernel
    (rac_regroup_fwd)."""
    B, T, N, C = dims
    _lib.require_gpu(*feats, what="regroup_pyramid")
    outs = [torch.empty(B * T * groups, N, f.shape[3], f.shape[4], C, device=f.device, dtype=out_dtype) for f in feats]
    code = _lib.RAC_F32 if out_dtype == torch.float32 else _lib.RAC_BF16
    if C % 4 == 0 and all((f.shape[3] * f.shape[4]) % 4 == 0 for f in feats) and len(feats) <= 8:
        L = len(feats)
        ins = (ctypes.c_void_p * L)(*[f.data_ptr() for f in feats])
        dst = (ctypes.c_void_p * L)(*[o.data_ptr() for o in outs])
        hw = (ctypes.c_int32 * (2 * L))(*[int(x) for f in feats for x in f.shape[3:5]])
        _lib.check(_lib.lib().rac_regroup_multi_fwd(L, ins, dst, hw, B, T, N, groups, C, code, _lib.stream_ptr()), "rac_regroup_multi_fwd")
        return outs
    for feat, dst in zip(feats, outs):
        H, W = feat.shape[3:5]
        _lib.check(_lib.lib().rac_regroup_fwd(_lib.ptr(feat), _lib.ptr(dst), B, T, N, groups, C, H, W, code, _lib.stream_ptr()),
                   "rac_regroup_fwd")
    return outs


def regroup_backward(grads, dims, groups):
    """Backward of regroup_fused, the inverse transposition: grads[l] float32 [B*T*G,N,H,W,C] (the levels that need a gradient
    only) -> [B,T*N,G*C,H,W], bit-exact, ONE launch (rac_regroup_multi_bwd; rac_regroup_bwd per level for sizes that are not
    multiples of 4)."""
    B, T, N, C = dims
    grads = [g.contiguous() for g in grads]
    _lib.require_gpu(*grads, what="regroup_backward")
    for g in grads:
        if g.dtype != torch.float32 or g.dim() != 5 or (g.shape[0], g.shape[1], g.shape[4]) != (B * T * groups, N, C):
            raise RuntimeError("regroup_backward: float32 features only, [B*T*G, N, H, W, C]")
    outs = [torch.empty(B, T * N, groups * C, g.shape[2], g.shape[3], device=g.device, dtype=torch.float32) for g in grads]
    if C % 4 == 0 and all((g.shape[2] * g.shape[3]) % 4 == 0 for g in grads) and len(grads) <= 8:
        L = len(grads)
        src = (ctypes.c_void_p * L)(*[g.data_ptr() for g in grads])
        dst = (ctypes.c_void_p * L)(*[o.data_ptr() for o in outs])
        hw = (ctypes.c_int32 * (2 * L))(*[int(x) for g in grads for x in g.shape[2:4]])
        _lib.check(_lib.lib().rac_regroup_multi_bwd(L, src, dst, hw, B, T, N, groups, C, _lib.stream_ptr()), "rac_regroup_multi_bwd")
        return outs
    for g, dst in zip(grads, outs):
        H, W = g.shape[2:4]
        _lib.check(_lib.lib().rac_regroup_bwd(_lib.ptr(g), _lib.ptr(dst), B, T, N, groups, C, H, W, _lib.stream_ptr()), "rac_regroup_bwd")
    return outs


SPLIT_ACT_SCALE = 16.0   # power of two applied to activations before the f16 hi/lo split (keeps lo out of f16 subnormals)
SPLIT_BIAS_PAD = 64      # extra K columns of a split image that carry the bias ([1, 1, 0...] against [b_hi, b_lo, 0...]);
                         # 3*256 + 64 = 832 = 13 x 64 keeps hipBLASLt on its fast kernels (776: 187 us, 832: 134 us)
SPLIT_SLICE = 2048       # K slice of out_proj's split-K (16 slices of the 32768-long reduction)


def head_finish_fused(cls_scores, bbox_xy, pc_range):
    """(nan_to_num(cls_scores) in place, boxes [..,10] = denormalised + reordered nan_to_num(bbox_xy)): the element-wise tail of
    RaCFormerTransformer.forward / RaCFormer_head.forward in one launch (rac_head_finish_fwd)."""
    _lib.require_gpu(cls_scores, bbox_xy, what="head_finish_fused")
    if cls_scores.dtype != torch.float32 or bbox_xy.dtype != torch.float32 or bbox_xy.shape[-1] != 10:
        raise RuntimeError("head_finish_fused: float32 tensors, boxes with 10 columns")
    box = torch.empty_like(bbox_xy)
    pc = (ctypes.c_float * 6)(*[float(v) for v in pc_range])
    rc = _lib.lib().rac_head_finish_fwd(_lib.ptr(cls_scores), cls_scores.numel(), _lib.ptr(bbox_xy), _lib.ptr(box), bbox_xy.numel() // 10, 10,
                                        pc, _lib.stream_ptr())
    _lib.check(rc, "rac_head_finish_fwd")
    return cls_scores, box


def layer_boundary_fused(proposal, delta, time_diff_safe, num_ray, pc_range, pe_linear, pe_norm, xy_out=None):
    """refine_fused + box_prep + pe_head for the refined boxes in one launch (rac_layer_boundary_fwd).
    -> (bbox_pred [B,Q,10], bbox_xy [B,Q,10], box_table [B,Q,8], pe_head output [B,Q,256])."""
    _boxes_and_times("layer_boundary_fused", proposal, delta, time_diff_safe)
    _pe_operands("layer_boundary_fused", pe_linear, pe_norm)
    proposal, delta = proposal.contiguous(), delta.contiguous()
    _lib.require_gpu(proposal, delta, time_diff_safe, pe_linear.weight, pe_linear.bias, pe_norm.weight, pe_norm.bias,
                     what="layer_boundary_fused")
    B, Q, _ = proposal.shape
    pred = torch.empty_like(proposal)
    if xy_out is None:
        xy = torch.empty_like(proposal)
    else:
        if tuple(xy_out.shape) != tuple(proposal.shape) or not xy_out.is_contiguous() or xy_out.dtype != torch.float32 \
                or not xy_out.is_cuda:
            raise RuntimeError("layer_boundary_fused: xy_out must be a contiguous float32 CUDA tensor shaped like the boxes")
        xy = xy_out
    table = torch.empty(B, Q, 8, device=proposal.device, dtype=torch.float32)
    h = torch.empty(B, Q, pe_linear.weight.shape[0], device=proposal.device, dtype=torch.float32)
    pc = (ctypes.c_float * 6)(*[float(v) for v in pc_range])
    rc = _lib.lib().rac_layer_boundary_fwd(_lib.ptr(proposal), _lib.ptr(delta), _lib.ptr(time_diff_safe), _lib.ptr(pred),
                                           _lib.ptr(xy), _lib.ptr(table), pc, _lib.ptr(pe_linear.weight), _lib.ptr(pe_linear.bias),
                                           _lib.ptr(pe_norm.weight), _lib.ptr(pe_norm.bias), _lib.ptr(h), B, Q,
                                           time_diff_safe.shape[1], pe_linear.weight.shape[0], float(num_ray), float(pe_norm.eps),
                                           _lib.stream_ptr())
    _lib.check(rc, "rac_layer_boundary_fwd")
    return pred, xy, table, h


def add_ln(a, norm, residual=None, bias=None, relu=False, num_partials=1, post=None, out=None, split=False, a_scale=1.0,
           split_lines=False, split_out=None):
    """[relu](LayerNorm(a_scale * sum_s a[s] + residual + bias)) [+ post] with ``norm`` an nn.LayerNorm; a is [..., dim]
    (unit inner stride; rows may be a column slice of a wider tensor) or [S, ..., dim] with num_partials=S.
    ``out``: optional destination (may itself be a column slice).  One launch.
    ``split=True``: also returns the f16 [rows, 3*dim + SPLIT_BIAS_PAD] = [hi | hi | lo | 1 1 0..] image of
    ``out * SPLIT_ACT_SCALE`` (A operand of a split GEMM, see ``split_weight_f16``); with ``split_lines`` the image is the
    line image [rows, dim/32 * 64] = [hi 32 | lo 32] per 32 columns that ``generator_fused`` reads."""
    dim = a.shape[-1]
    if num_partials > 1:
        if a.dim() < 2 or a.shape[0] != num_partials:
            raise RuntimeError(f"add_ln: a must be [{num_partials}, ..., dim] with num_partials={num_partials}, got {tuple(a.shape)}")
        rows = a.numel() // dim // num_partials
    else:
        rows = int(torch.Size(a.shape[:-1]).numel())
    # the kernels read rows * dim elements of residual / post and dim of bias, gamma and beta, whatever the tensors hold
    _sized("add_ln", "residual", residual, rows * dim, f"rows * dim = {rows} * {dim}")
    _sized("add_ln", "post", post, rows * dim, f"rows * dim = {rows} * {dim}")
    _sized("add_ln", "bias", bias, dim, f"dim = {dim}")
    _sized("add_ln", "norm.weight", norm.weight, dim, f"dim = {dim}")
    _sized("add_ln", "norm.bias", norm.bias, dim, f"dim = {dim}")
    if a.dtype != torch.float32:
        raise RuntimeError(f"add_ln: a must be float32, got {a.dtype}")
    if out is not None:
        if out.dtype != torch.float32 or out.dim() < 1 or out.stride(-1) != 1 or out.shape[-1] != dim or out.numel() != rows * dim:
            raise RuntimeError(f"add_ln: out must be a float32 [{rows} rows, {dim}] view with unit inner stride, got {tuple(out.shape)}")
        if any(out.stride(i) != out.shape[i + 1] * out.stride(i + 1) for i in range(out.dim() - 2)):
            raise RuntimeError("add_ln: out's rows must be equally strided")
    if num_partials > 1:
        a = a.contiguous()
        ld_a, shape = dim, a.shape[1:]
    else:
        if a.stride(-1) != 1 or not a.is_cuda:
            raise RuntimeError("add_ln: input must be a CUDA tensor with unit inner stride")
        shape = a.shape
        ld_a = a.stride(-2) if a.dim() > 1 else dim
        if a.dim() > 2 and a.stride(0) != a.shape[1] * a.stride(1):
            raise RuntimeError("add_ln: rows must be equally strided")
    if residual is not None:
        residual = residual.contiguous()
        shape = residual.shape
    if post is not None:
        post = post.contiguous()
    # every pointer the kernel takes is a device pointer (contiguous where the kernel assumes it)
    _lib.require_gpu(norm.weight, norm.bias, *[t for t in (residual, post, bias) if t is not None],
                     *([a] if num_partials > 1 else []), what="add_ln")
    if out is None:
        out = torch.empty(shape, device=a.device, dtype=torch.float32)
        ld_out = dim
    else:
        if not out.is_cuda:
            raise RuntimeError("racformer_amd.add_ln: out must be a CUDA tensor (HIP device); the hot path has no CPU fallback")
        ld_out = out.stride(-2) if out.dim() > 1 else dim
    if split:
        width = 2 * dim if split_lines else 3 * dim + SPLIT_BIAS_PAD
        if split_out is None:
            split_out = torch.empty(rows, width, device=a.device, dtype=torch.float16)
        elif split_out.dtype != torch.float16 or not split_out.is_contiguous() or tuple(split_out.shape) != (rows, width) \
                or not split_out.is_cuda:
            raise RuntimeError(f"add_ln: split_out must be a contiguous f16 CUDA [{rows}, {width}] tensor")
    rc = _lib.lib().rac_add_ln_fwd(_lib.ptr(a), num_partials, rows * dim, ld_a, float(a_scale),
                                   _lib.ptr(residual) if residual is not None else None,
                                   _lib.ptr(bias) if bias is not None else None, _lib.ptr(norm.weight), _lib.ptr(norm.bias),
                                   _lib.ptr(post) if post is not None else None, _lib.ptr(out), ld_out, rows, dim,
                                   float(norm.eps), int(relu), _lib.ptr(split_out) if split else None,
                                   SPLIT_ACT_SCALE, 0 if split_lines else SPLIT_BIAS_PAD, 1 if split_lines else 0, _lib.stream_ptr())
    _lib.check(rc, "rac_add_ln_fwd")
    return (out, split_out) if split else out


def split_weight_f16(weight, bias=None):
    """nn.Linear weight [N,K] fp32 -> (f16 [N,3K] = [hi | lo | hi] of weight * 2^s, alpha) such that
        x @ weight.T  ==  alpha * ([x_hi | x_hi | x_lo] @ [w_hi | w_lo | w_hi].T)        (x * SPLIT_ACT_SCALE = x_hi + x_lo)
    up to the dropped lo*lo term (2^-22 relative): fp32-GEMM accuracy from three f16 MFMA products accumulated in
    fp32.  2^s brings max|w| to [2^13, 2^14) so that the lo parts stay clear of f16 subnormals; alpha undoes both
    power-of-two scalings exactly.  With ``bias`` the image is [N, 3K + SPLIT_BIAS_PAD] = [.. | b_hi | b_lo | 0..]
    (bias * 2^s): against the [.. | 1 | 1 | 0..] columns of add_ln's activation image the GEMM adds the bias
    itself.  Done once per set of weights (the caller caches it).  (None, None) if f16 cannot hold the operands."""
    import math
    w = weight.detach().float()
    amax = float(w.abs().max())
    if not (amax > 0.0) or amax != amax or amax == float("inf"):
        return None, None
    s = 13 - math.frexp(amax)[1] + 1          # amax * 2^s in [2^13, 2^14)
    ws = w * (2.0 ** s)
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)
    parts = [hi, lo, hi]
    if bias is not None:
        bs = bias.detach().float() * (2.0 ** s)
        if not float(bs.abs().max()) < 6.0e4:
            return None, None
        bh = bs.to(torch.float16)
        bl = (bs - bh.float()).to(torch.float16)
        parts += [bh[:, None], bl[:, None], hi.new_zeros(hi.shape[0], SPLIT_BIAS_PAD - 2)]
    return torch.cat(parts, dim=1).contiguous(), 2.0 ** (-s) / SPLIT_ACT_SCALE


def pe_head(x3, linear, norm):
    """relu(LayerNorm(linear(x3))) for the 3-wide position-encoder input, one launch.  x3: [..., 3] view."""
    if x3.dim() < 2 or x3.shape[-1] != 3 or x3.dtype != torch.float32:
        raise RuntimeError(f"pe_head: x3 must be a float32 [..., 3] view, got {tuple(x3.shape)}")
    _pe_operands("pe_head", linear, norm)
    if x3.stride(-1) != 1 or not x3.is_cuda:
        raise RuntimeError("pe_head: input must be a CUDA tensor with unit inner stride")
    if x3.dim() > 2 and any(x3.stride(i) != x3.shape[i + 1] * x3.stride(i + 1) for i in range(x3.dim() - 2)):
        raise RuntimeError("pe_head: rows must be equally strided")
    _lib.require_gpu(linear.weight, linear.bias, norm.weight, norm.bias, what="pe_head")
    rows = int(torch.Size(x3.shape[:-1]).numel())
    out = torch.empty(x3.shape[:-1] + (linear.weight.shape[0],), device=x3.device, dtype=torch.float32)
    rc = _lib.lib().rac_pe_head_fwd(_lib.ptr(x3), x3.stride(-2), _lib.ptr(linear.weight), _lib.ptr(linear.bias),
                                    _lib.ptr(norm.weight), _lib.ptr(norm.bias), _lib.ptr(out), rows, linear.weight.shape[0],
                                    float(norm.eps), _lib.stream_ptr())
    _lib.check(rc, "rac_pe_head_fwd")
    return out


# ------------------------------------------------------------------------------------------- 3x3 convolution
def pack_conv3x3_weight(weight, cout=256):
    """nn.Conv2d weight [cout, Cin, 3, 3] fp32 -> (ws f16 [9, Cin/32, cout, 2, 32], w_alpha) for rac_conv3x3_fwd (cout 256) /
    rac_conv3x3s2_fwd (cout 64):
    hi / lo of weight * 2^s per (tap, 32-channel chunk, output channel), w_alpha = 2^-s.  (None, None) if the
    weights cannot be held."""
    import math
    w = weight.detach().float()
    co, ci, kh, kw = w.shape
    amax = float(w.abs().max())
    if (kh, kw) != (3, 3) or co != cout or ci % 32 != 0 or not (amax > 0.0) or amax != amax or amax == float("inf"):
        return None, None
    s = 13 - math.frexp(amax)[1] + 1
    ws = (w * (2.0 ** s)).permute(2, 3, 1, 0).reshape(9, ci // 32, 32, co).permute(0, 1, 3, 2)      # [tap, chunk, co, 32]
    hi = ws.to(torch.float16)
    lo = (ws - hi.float()).to(torch.float16)
    return torch.stack([hi, lo], dim=3).contiguous(), 2.0 ** (-s)


def conv3x3_dgrad_weight(weight):
    """The weights of the data gradient of a 3x3 / stride 1 / pad 1 convolution, itself such a convolution of the output gradient:
    W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx].  weight [Cout, Cin, 3, 3] -> [Cin, Cout, 3, 3]."""
    return weight.detach().flip(2, 3).transpose(0, 1).contiguous()


def pack_conv3x3_dgrad_weight(weight, c0=0, cout=256):
    """pack_conv3x3_weight of the rows [c0, c0 + cout) of conv3x3_dgrad_weight(weight) -- the gradient of ``cout`` input channels
    per launch of rac_conv3x3_fwd on an image of the output gradient.  Where fewer than ``cout`` input channels remain the
    image gets zero output columns: -> (ws, w_alpha, rows) with ``rows`` the number of real ones ((None, None, 0) if the weights
    cannot be held, an all-zero slice included).
    Accuracy of the image, as of pack_conv3x3_weight's: hi + lo = w' * 2^s to 2^-22 relative per element (two 11-bit halves),
    plus at most 2^-25 of the scaled unit where lo falls below f16's subnormal step 2^-24 -- with the largest |w'| * 2^s in
    [2^13, 2^14) that absolute term is below 2^-38 of the largest weight."""
    wt = conv3x3_dgrad_weight(weight)[c0:c0 + cout].float()
    rows = int(wt.shape[0])
    if 0 < rows < cout:
        wt = torch.cat([wt, wt.new_zeros((cout - rows,) + tuple(wt.shape[1:]))], dim=0)
    ws, alpha = pack_conv3x3_weight(wt, cout=cout) if rows > 0 else (None, None)
    return (ws, alpha, rows) if ws is not None else (None, None, 0)


def unpack_conv3x3_weight(ws, w_alpha):
    """Inverse of pack_conv3x3_weight up to the split's rounding: (ws [9, Cin/32, cout, 2, 32] f16, w_alpha) -> [cout, Cin, 3, 3] float64."""
    v = (ws[:, :, :, 0].double() + ws[:, :, :, 1].double()) * float(w_alpha)          # [tap, chunk, co, 32]
    taps, chunks, co, _ = v.shape
    return v.permute(2, 1, 3, 0).reshape(co, chunks * 32, 3, 3)


def wgrad_k_splits(N, H, W, cin):
    """Number of K ranges of rac_conv3x3_wgrad for a shape: about 512 workgroups (two per CU) over the 2 * cin / 32 output tiles,
    at most one range per image row, none empty.  A function of the shape alone, so a shape always sums in the same order."""
    rows = N * H
    want = max(1, min(rows, 512 // max(1, 2 * (cin // 32))))
    per = -(-rows // want)
    return -(-rows // per)


_conv_images = {}
_scratch_ns = [None]


class scratch_namespace:
    """Reusable device scratch (the convolution kernels' activation images) is shared by every forward of a process -- fine while
    forwards follow each other on one stream.  A captured plan that is replayed BESIDE another one (racformer_amd/graph.py, several
    samples in flight on streams of their own) has to own its scratch: forwards run inside ``with scratch_namespace(key)`` get
    buffers of that namespace."""

    def __init__(self, key):
        self.key = key

    def __enter__(self):
        self.prev, _scratch_ns[0] = _scratch_ns[0], self.key
        return self

    def __exit__(self, *exc):
        _scratch_ns[0] = self.prev


def release_scratch(key):
    """Drops the scratch buffers of a namespace (a captured plan that owned them is gone)."""
    for k in [k for k in _conv_images if k[-1] == key]:
        del _conv_images[k]


class ConvImage:
    """The padded channel-last f16 hi/lo activation image of the convolution kernels, filled in stages:
    ``begin`` (absmax -> the activations' power-of-two scale), ``pack`` (NCHW fp32 source -> a channel range), then
    ``conv`` (3x3 stride 1 -> [N,H,W,256] channel-last) and / or ``conv_s2`` (3x3 stride 2 over the first channels ->
    [N,64,H/2,W/2]).  The buffer (zero border = the convolutions' padding) is allocated once per shape and reused."""

    def __init__(self, N, H, W, cin, device):
        self.N, self.H, self.W, self.cin, self.dev = N, H, W, cin, device
        key = (N, H, W, cin, str(device), _scratch_ns[0])
        xs = _conv_images.get(key)
        if xs is None:
            xs = _conv_images[key] = torch.zeros(N, H + 2, W + 2, cin // 32, 2, 32, device=device, dtype=torch.float16)
        self.xs = xs
        self.amax = torch.empty(1, device=device, dtype=torch.float32)

    def begin(self, scan, floor=0.0):
        """amax = max(floor, max |v| over the tensors in ``scan``); every source packed later must be covered by it."""
        n = len(scan)
        _lib.require_gpu(*scan, what="ConvImage.begin")
        ptrs = (ctypes.c_void_p * max(n, 1))(*[t.data_ptr() for t in scan])
        counts = (ctypes.c_int64 * max(n, 1))(*[t.numel() for t in scan])
        _lib.check(_lib.lib().rac_absmax_fwd(ptrs, counts, n, float(floor), _lib.ptr(self.amax), _lib.stream_ptr()),
                   "rac_absmax_fwd")
        return self

    def pack(self, src, c_offset):
        _lib.require_gpu(src, what="ConvImage.pack")
        if tuple(src.shape[0:1] + src.shape[2:]) != (self.N, self.H, self.W) or src.dtype != torch.float32:
            raise RuntimeError("ConvImage.pack: sources must be float32 [N,C,H,W] matching the image")
        _lib.check(_lib.lib().rac_conv_pack_fwd(_lib.ptr(src), _lib.ptr(self.amax), _lib.ptr(self.xs), self.N, int(src.shape[1]),
                                                self.H, self.W, self.cin, int(c_offset), _lib.stream_ptr()), "rac_conv_pack_fwd")
        return self

    def pack_cl(self, src, c_offset):
        """``pack`` for a channel-last source [N,H,W,C] (rac_conv_pack_cl_fwd)."""
        _lib.require_gpu(src, what="ConvImage.pack_cl")
        if tuple(src.shape[:3]) != (self.N, self.H, self.W) or src.dtype != torch.float32 or not src.is_contiguous():
            raise RuntimeError("ConvImage.pack_cl: sources must be contiguous float32 [N,H,W,C] matching the image")
        _lib.check(_lib.lib().rac_conv_pack_cl_fwd(_lib.ptr(src), _lib.ptr(self.amax), _lib.ptr(self.xs), self.N, int(src.shape[3]),
                                                   self.H, self.W, self.cin, int(c_offset), _lib.stream_ptr()), "rac_conv_pack_cl_fwd")
        return self

    def pack_live(self, src, bias, c_offset, frames_per_group):
        """Channel range [c_offset, c_offset + C) from ``src`` [G * live, C, H, W] (+ per-channel ``bias``) where the image's N frames
        come in G groups of ``frames_per_group`` and only the first ``live`` of a group exist in src; the others are the bias alone
        (rac_conv_pack_bias_fwd)."""
        _lib.require_gpu(src, what="ConvImage.pack_live")
        G = self.N // frames_per_group
        if self.N % frames_per_group != 0 or src.shape[0] % G != 0 or tuple(src.shape[2:]) != (self.H, self.W) or src.dtype != torch.float32:
            raise RuntimeError("ConvImage.pack_live: src must be float32 [groups * live, C, H, W] matching the image")
        _lib.check(_lib.lib().rac_conv_pack_bias_fwd(_lib.ptr(src), _lib.ptr(bias) if bias is not None else None, _lib.ptr(self.amax),
                                                     _lib.ptr(self.xs), self.N, int(src.shape[1]), self.H, self.W, self.cin, int(c_offset),
                                                     int(frames_per_group), int(src.shape[0] // G), _lib.stream_ptr()),
                   "rac_conv_pack_bias_fwd")
        return self

    def conv(self, ws, w_alpha, bias=None, pixel_bias=None, q16=False):
        """-> [N,H,W,256] fp32 channel-last, or with ``q16`` the same result in the int16 block storage of quantize_values_i16
        (q int16 [N, H*W, 4, 64], scale f32 [N, H*W, 4]), quantised in the kernel's epilogue (rac_conv3x3_q16_fwd)."""
        N, H, W = self.N, self.H, self.W
        if pixel_bias is not None and (tuple(pixel_bias.shape) != (H * W, 256) or not pixel_bias.is_contiguous()
                                       or pixel_bias.dtype != torch.float32 or not pixel_bias.is_cuda):
            raise RuntimeError("ConvImage.conv: pixel_bias must be a contiguous float32 CUDA [H*W, 256] tensor")
        if q16:
            out = torch.empty(N, H * W, 4, 64, device=self.dev, dtype=torch.int16)
            scale = torch.empty(N, H * W, 4, device=self.dev, dtype=torch.float32)
        else:
            out = torch.empty(N, H, W, 256, device=self.dev, dtype=torch.float32)
        ev = _lib.timer.record("temporal_fusion_conv") if _lib.timer is not None else None
        if ev:
            ev[0].record()
        head = (_lib.ptr(self.xs), _lib.ptr(ws), _lib.ptr(bias) if bias is not None else None,
                _lib.ptr(pixel_bias) if pixel_bias is not None else None, _lib.ptr(self.amax), float(w_alpha))
        tail = (N, H, W, self.cin, 256, _lib.stream_ptr())
        if q16:
            rc, what = _lib.lib().rac_conv3x3_q16_fwd(*head, _lib.ptr(out), _lib.ptr(scale), *tail), "rac_conv3x3_q16_fwd"
        else:
            rc, what = _lib.lib().rac_conv3x3_fwd(*head, _lib.ptr(out), *tail), "rac_conv3x3_fwd"
        if ev:
            ev[1].record()
        _lib.check(rc, what)
        return (out, scale) if q16 else out

    def conv_temporal(self, ws, w_alpha, pixel_bias_live, pixel_bias_dead, cin_dead, frames_per_group, live_per_group, q16=False):
        """``conv`` for a stack of [groups, frames_per_group] images whose frames past the first ``live_per_group`` of a group carry a
        per-channel CONSTANT in the channels from ``cin_dead`` on: those images multiply only their first ``cin_dead`` channels and add
        ``pixel_bias_dead`` (the constant's contribution through the zero padding, folded in by the caller) instead of
        ``pixel_bias_live`` (rac_conv3x3_temporal_fwd).  Same outputs as ``conv``."""
        N, H, W = self.N, self.H, self.W
        for pb in (pixel_bias_live, pixel_bias_dead):
            if tuple(pb.shape) != (H * W, 256) or not pb.is_contiguous() or pb.dtype != torch.float32 or not pb.is_cuda:
                raise RuntimeError("ConvImage.conv_temporal: the per-pixel maps must be contiguous float32 CUDA [H*W, 256] tensors")
        if q16:
            out = torch.empty(N, H * W, 4, 64, device=self.dev, dtype=torch.int16)
            scale = torch.empty(N, H * W, 4, device=self.dev, dtype=torch.float32)
        else:
            out, scale = torch.empty(N, H, W, 256, device=self.dev, dtype=torch.float32), None
        ev = _lib.timer.record("temporal_fusion_conv") if _lib.timer is not None else None
        if ev:
            ev[0].record()
        rc = _lib.lib().rac_conv3x3_temporal_fwd(_lib.ptr(self.xs), _lib.ptr(ws), _lib.ptr(pixel_bias_live), _lib.ptr(pixel_bias_dead),
                                                 _lib.ptr(self.amax), float(w_alpha), None if q16 else _lib.ptr(out),
                                                 _lib.ptr(out) if q16 else None, _lib.ptr(scale) if q16 else None, N, H, W, self.cin,
                                                 int(cin_dead), int(frames_per_group), int(live_per_group), _lib.stream_ptr())
        if ev:
            ev[1].record()
        _lib.check(rc, "rac_conv3x3_temporal_fwd")
        return (out, scale) if q16 else out

    def conv_s2(self, ws, w_alpha, bias, cin, out=None):
        """3x3 / stride 2 / pad 1 convolution of the image's first ``cin`` channels -> [N, 64, H/2, W/2] fp32 (NCHW), or
        into channels 0..63 of a given contiguous ``out`` [N, Ctot, H/2, W/2]."""
        N, H, W = self.N, self.H, self.W
        if out is None:
            out = torch.empty(N, 64, H // 2, W // 2, device=self.dev, dtype=torch.float32)
        elif not out.is_contiguous() or tuple(out.shape[0:1] + out.shape[2:]) != (N, H // 2, W // 2) or out.shape[1] < 64:
            raise RuntimeError("ConvImage.conv_s2: out must be a contiguous [N, >=64, H/2, W/2] tensor")
        _lib.check(_lib.lib().rac_conv3x3s2_fwd(_lib.ptr(self.xs), _lib.ptr(ws), _lib.ptr(bias) if bias is not None else None,
                                                _lib.ptr(self.amax), float(w_alpha), _lib.ptr(out), int(out.shape[1]), N, H, W,
                                                int(cin), self.cin, 64, _lib.stream_ptr()), "rac_conv3x3s2_fwd")
        return out


def conv3x3_wgrad(x_img, g_img, k_splits=None):
    """Weight gradient [256, Cin, 3, 3] fp32 of the 3x3 / stride 1 / pad 1 convolution from the packed images of its input
    (``x_img``, Cin channels) and of its output gradient (``g_img``, 256 channels): rac_conv3x3_wgrad, partial sums per range of
    image rows added in a fixed order."""
    N, H, W = x_img.N, x_img.H, x_img.W
    if (g_img.N, g_img.H, g_img.W, g_img.cin) != (N, H, W, 256):
        raise RuntimeError("conv3x3_wgrad: the gradient image must be [N,H,W] of 256 channels like the input image")
    k = wgrad_k_splits(N, H, W, x_img.cin) if k_splits is None else int(k_splits)
    work = torch.empty(k, 9, 256, x_img.cin, device=x_img.dev, dtype=torch.float32)
    dw = torch.empty(256, x_img.cin, 3, 3, device=x_img.dev, dtype=torch.float32)
    _lib.check(_lib.lib().rac_conv3x3_wgrad(_lib.ptr(x_img.xs), _lib.ptr(g_img.xs), _lib.ptr(x_img.amax), _lib.ptr(g_img.amax),
                                            _lib.ptr(work), _lib.ptr(dw), N, H, W, x_img.cin, 256, k, _lib.stream_ptr()),
               "rac_conv3x3_wgrad")
    return dw


def temporal_fusion_forward(x, hid, ws, w_alpha, bias):
    """conv3x3(cat[x, hid]) + bias -> [N,H,W,256] fp32 channel-last: both halves packed into one image, no concatenation."""
    N, cx, H, W = x.shape
    img = ConvImage(N, H, W, cx + int(hid.shape[1]), x.device)
    img.begin([x, hid]).pack(x, 0).pack(hid, cx)
    return img.conv(ws, w_alpha, bias)


def _zero_dgrad(w_slice, like):
    """The data gradient through a weight slice pack_conv3x3_weight could not hold: zeros where the slice is all zero (e.g. a
    zero-initialised hidden half); anything else (inf, NaN) is an error, not something to paper over."""
    if bool((w_slice.detach() != 0).any()):
        raise RuntimeError("temporal_fusion_backward: the transposed weights cannot be packed (non-finite values)")
    return torch.zeros_like(like)


def temporal_fusion_backward(x, hid, weight, grad_out, need_x, need_hid, need_w, packs):
    """Gradients of temporal_fusion_forward: grad_out [N,H,W,256] channel-last -> (grad_x [N,256,H,W], grad_hid [N,hidden,H,W],
    grad_w [256,Cin,3,3]; None where not asked for).  ``packs``: a dict that keeps the packed transposed weights ("dx", "dh")
    for the weights' lifetime.  The image of grad_out gets its scale from its own maximum; the data gradients are
    rac_conv3x3_fwd launches on it (views of channel-last results), the weight gradient rac_conv3x3_wgrad on it and the re-packed
    image of the input."""
    N, cx, H, W = x.shape
    hd = int(hid.shape[1])
    g_img = ConvImage(N, H, W, 256, x.device)
    g_img.begin([grad_out]).pack_cl(grad_out, 0)
    gx = gh = gw = None
    if need_x:
        if "dx" not in packs:
            packs["dx"] = pack_conv3x3_dgrad_weight(weight, 0)
        ws, alpha, _ = packs["dx"]
        # (an all-zero slice of the weights has no power-of-two scale to pack with: its data gradient is exactly zero)
        gx = g_img.conv(ws, alpha).permute(0, 3, 1, 2) if ws is not None else _zero_dgrad(weight[:, :cx], x)
    if need_hid:
        if "dh" not in packs:
            packs["dh"] = pack_conv3x3_dgrad_weight(weight, cx)
        ws, alpha, _ = packs["dh"]
        gh = g_img.conv(ws, alpha)[..., :hd].permute(0, 3, 1, 2) if ws is not None else _zero_dgrad(weight[:, cx:], hid)
    if need_w:
        x_img = ConvImage(N, H, W, cx + hd, x.device)
        x_img.begin([x, hid]).pack(x, 0).pack(hid, cx)
        gw = conv3x3_wgrad(x_img, g_img)
    return gx, gh, gw


def conv3x3_fused(sources, ws, w_alpha, bias, bounds=None, pixel_bias=None):
    """3x3 / stride 1 / pad 1 convolution of the channel concatenation of ``sources`` (NCHW fp32 tensors with
    equal N, H, W) -> [N, H, W, 256] fp32 channel-last: ConvImage.begin -> pack ... -> conv in one call.
    ``bounds[i]``: a known upper bound of |sources[i]| (the source is then not scanned by the absmax pass).
    ``pixel_bias``: [H*W, 256] additive map (per pixel and output channel, shared by the N images) instead of ``bias``."""
    _lib.require_gpu(*sources, ws, what="conv3x3_fused")
    N, _, H, W = sources[0].shape
    cin = sum(int(t.shape[1]) for t in sources)
    bounds = list(bounds) if bounds is not None else [None] * len(sources)
    img = ConvImage(N, H, W, cin, sources[0].device)
    img.begin([t for t, bnd in zip(sources, bounds) if bnd is None], max([0.0] + [float(b) for b in bounds if b is not None]))
    off = 0
    for t in sources:
        img.pack(t, off)
        off += int(t.shape[1])
    return img.conv(ws, w_alpha, bias, pixel_bias)


# ------------------------------------------------------------------------------------------- ConvGRU branch, own kernels (round 5)
def act_image(tag, frames, H, W, channels, device):
    """A zero-bordered activation image f16 [frames, H+2, W+2, channels/32, 2, 32] of the convolution kernels, from the reusable
    scratch of the current namespace (scratch_namespace): allocated zeroed once per (tag, shape); its producers write interior
    pixels only, so the border stays the convolutions' zero padding."""
    key = ("act", tag, frames, H, W, channels, str(device), _scratch_ns[0])
    img = _conv_images.get(key)
    if img is None:
        img = _conv_images[key] = torch.zeros(frames, H + 2, W + 2, channels // 32, 2, 32, device=device, dtype=torch.float16)
    return img


def _cd_scale(amax=None, mul=0.0, add=0.0):
    return _lib.CdScale(_lib.ptr(amax) if amax is not None else None, float(mul), float(add))


def _cd_frames(live=1, stride=1, first=0):
    return _lib.CdFrames(int(live), int(stride), int(first))


def conv_direct(mode, N, H, W, in_img, in_chunks_total, chunks, ws, w_alpha, cout, in_scale, conv_stride=1, in_chunk0=0,
                in_frames=None, bias=None, out_img=None, out_chunks_total=0, out_chunk0=0, out_frames=None, out_scale=None,
                out_f32=None, pixel_map=None, xpart=None, xpart_frames=None, h_prev=None, h_prev_frames=None, h_out=None,
                h_out_frames=None):
    """rac_conv_direct_fwd (include/racformer_hip.h): 3x3 convolution of a small activation image without LDS staging, epilogue
    ``mode`` = _lib.CD_IMAGE (another activation image) / CD_F32 (channel-last fp32 + per-pixel map) / CD_GRU (the ConvGRU update).
    Scales are (amax tensor | None, mul, add) triples, frame maps (live, stride, first) triples."""
    opt = lambda t: _lib.ptr(t) if t is not None else None      # noqa: E731
    fr = lambda f: _cd_frames(*(f or (1, 1, 0)))                # noqa: E731
    d = _lib.ConvDirect()
    d.mode, d.conv_stride, d.N, d.H, d.W = int(mode), int(conv_stride), int(N), int(H), int(W)
    d.in_img, d.in_chunks_total, d.in_chunk0, d.chunks = opt(in_img), int(in_chunks_total), int(in_chunk0), int(chunks)
    d.in_frames, d.in_scale = fr(in_frames), _cd_scale(*in_scale)
    d.ws, d.w_alpha, d.Cout, d.bias = opt(ws), float(w_alpha), int(cout), opt(bias)
    d.out_img, d.out_chunks_total, d.out_chunk0 = opt(out_img), int(out_chunks_total), int(out_chunk0)
    d.out_frames, d.out_scale = fr(out_frames), _cd_scale(*(out_scale or (None, 0.0, 0.0)))
    d.out_f32, d.pixel_map = opt(out_f32), opt(pixel_map)
    d.xpart, d.xpart_frames = opt(xpart), fr(xpart_frames)
    d.h_prev, d.h_prev_frames = opt(h_prev), fr(h_prev_frames)
    d.h_out, d.h_out_frames = opt(h_out), fr(h_out_frames)
    for t in (in_img, ws, bias, out_img, out_f32, pixel_map, xpart, h_prev, h_out):
        if t is not None:
            _lib.require_gpu(t, what="conv_direct")
    _lib.check(_lib.lib().rac_conv_direct_fwd(ctypes.byref(d), _lib.stream_ptr()), "rac_conv_direct_fwd")


def upsample2x_image(src, img, bound):
    """nn.Upsample(x2, bilinear, align_corners=True) of channel-last maps ``src`` f32 [frames, h*w, C] (given as [frames, h, w, C])
    into the activation image ``img`` [frames, 2h+2, 2w+2, C/32, 2, 32] with the scale of ``bound`` (rac_upsample2x_image_fwd)."""
    _lib.require_gpu(src, img, what="upsample2x_image")
    frames, h, w, C = src.shape
    if tuple(img.shape) != (frames, 2 * h + 2, 2 * w + 2, C // 32, 2, 32) or img.dtype != torch.float16 or src.dtype != torch.float32:
        raise RuntimeError("upsample2x_image: src f32 [frames,h,w,C], img f16 [frames,2h+2,2w+2,C/32,2,32] expected")
    _lib.check(_lib.lib().rac_upsample2x_image_fwd(_lib.ptr(src), _lib.ptr(img), frames, h, w, C, float(bound), _lib.stream_ptr()),
               "rac_upsample2x_image_fwd")
    return img


# ------------------------------------------------------------------------------------------- temporal encoder pieces
def gru_gate_fused(gates, h_prev, h_out, bias_map=None, h_out2=None):
    """ConvGRUCell's element-wise update, one launch: gates [B,3C,H,W] contiguous; h_prev / h_out (/ h_out2) [B,C,H,W]
    views whose per-batch blocks are contiguous (e.g. the [:, t] slot of a [B,T,C,H,W] tensor).  ``bias_map`` [3C,H,W]
    is added to the gates first.  Writes h_out (and h_out2)."""
    B, C3, H, W = gates.shape
    C = C3 // 3
    if bias_map is not None and (tuple(bias_map.shape) != (C3, H, W) or not bias_map.is_contiguous() or not bias_map.is_cuda):
        raise RuntimeError("gru_gate_fused: bias_map must be a contiguous CUDA [3C,H,W] tensor")
    for t in (h_prev, h_out) + ((h_out2,) if h_out2 is not None else ()):
        if not t.is_cuda or tuple(t.shape) != (B, C, H, W) or t[0].is_contiguous() is False or t.dtype != torch.float32:
            raise RuntimeError("gru_gate_fused: h_prev / h_out must be float32 CUDA [B,C,H,W] views with contiguous batches")
    _lib.require_gpu(gates, what="gru_gate_fused")
    bs = lambda t: t.stride(0) if B > 1 else C * H * W   # noqa: E731
    rc = _lib.lib().rac_gru_gate_fwd(_lib.ptr(gates), _lib.ptr(h_prev), bs(h_prev), _lib.ptr(h_out), bs(h_out),
                                     _lib.ptr(bias_map) if bias_map is not None else None,
                                     _lib.ptr(h_out2) if h_out2 is not None else None, bs(h_out2) if h_out2 is not None else 0,
                                     B, C, H * W, _lib.stream_ptr())
    _lib.check(rc, "rac_gru_gate_fwd")
    return h_out


def upsample2x_fused(x):
    """nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True) on a contiguous [N,C,h,w] tensor, one launch."""
    _lib.require_gpu(x, what="upsample2x_fused")
    N, C, h, w = x.shape
    out = torch.empty(N, C, 2 * h, 2 * w, device=x.device, dtype=torch.float32)
    rc = _lib.lib().rac_upsample2x_fwd(_lib.ptr(x), _lib.ptr(out), N * C, h, w, _lib.stream_ptr())
    _lib.check(rc, "rac_upsample2x_fwd")
    return out


# ------------------------------------------------------------------------------------------- row GEMMs
def _rows2d(t, what):
    """-> (tensor kept alive, pointer, row stride) of a float32 [rows, W] / [B, Q, W] view with unit inner stride (rowgemm_launch
    refuses anything that is not on the GPU)."""
    if t.dtype != torch.float32 or t.stride(-1) != 1:
        raise RuntimeError(f"racformer_amd.rowgemm({what}): expected a float32 tensor with unit inner stride")
    if t.dim() == 3:
        if t.stride(0) != t.shape[1] * t.stride(1):
            raise RuntimeError(f"racformer_amd.rowgemm({what}): rows must be equally strided")
        ld = t.stride(1)
    elif t.dim() == 2:
        ld = t.stride(0)
    else:
        raise RuntimeError(f"racformer_amd.rowgemm({what}): expected [rows, W] or [B, Q, W]")
    return t, ctypes.c_void_p(t.data_ptr()), int(ld)


def row_seg(a, num_partials=1, a_scale=1.0, bias0=None, residual=None, norm=None, relu=False, post=None, x_out=None,
            split_out=None, split_lines=False):
    """One 256-wide segment of a rowgemm's A operand (see rac_rowgemm_fwd):
    [relu](LN_norm(a_scale * sum_p a[p] + bias0 + residual)) [+ post]; ``a`` is [rows,256] (any row stride) or, with
    num_partials = S > 1, a contiguous [S, rows, 256].  ``x_out`` / ``split_out``: destinations for the finished rows
    (fp32 [rows,256] / f16 [rows, 768 + SPLIT_BIAS_PAD] for a K-concatenated library GEMM, or -- ``split_lines`` -- the f16
    line image [rows, 8, hi 32 | lo 32] that ``generator_fused`` reads).
    Every operand's width is checked here, before a pointer is taken; the rows each one holds are kept for rowgemm_launch,
    which knows how many the kernel reads.  The description is for rowgemm_launch only: neither the row counts nor the device of
    its tensors have been checked yet, so it is not safe to hand to rac_rowgemm_fwd directly."""
    who = "row_seg"
    held = {}
    if num_partials > 1:
        if a.dim() < 2 or not a.is_contiguous() or a.shape[0] != num_partials or a.shape[-1] != 256 or a.dtype != torch.float32:
            raise RuntimeError(f"row_seg: a (partials) must be a contiguous float32 [{num_partials}, rows, 256] tensor, got {tuple(a.shape)}")
        held["a"] = a.numel() // num_partials // 256
    else:
        held["a"] = _row_operand(who, "a", a)
    for name, t in (("residual", residual), ("post", post), ("x_out", x_out)):
        if t is not None:
            held[name] = _row_operand(who, name, t)
    _sized(who, "bias0", bias0, 256, "256")
    if norm is not None:
        _sized(who, "norm.weight", norm.weight, 256, "256")
        _sized(who, "norm.bias", norm.bias, 256, "256")
    if split_out is not None:
        width = 512 if split_lines else 768 + SPLIT_BIAS_PAD
        if split_out.dtype != torch.float16 or not split_out.is_contiguous() or split_out.shape[-1] != width:
            raise RuntimeError(f"row_seg: split_out must be a contiguous f16 [rows, {width}] tensor")
        held["split_out"] = split_out.numel() // width
    g = _lib.RowSeg()
    keep = []
    if num_partials > 1:
        g.a, g.ld_a, g.partial_stride = ctypes.c_void_p(a.data_ptr()), 256, a.numel() // num_partials
        keep.append(a)
    else:
        t, g.a, g.ld_a = _rows2d(a, "a")
        g.partial_stride = 0
        keep.append(t)
    g.num_partials, g.a_scale, g.relu = num_partials, float(a_scale), int(relu)
    if bias0 is not None:
        g.bias0 = ctypes.c_void_p(bias0.data_ptr())
        keep.append(bias0)
    if residual is not None:
        t, g.residual, g.ld_res = _rows2d(residual, "residual")
        keep.append(t)
    if norm is not None:
        g.gamma, g.beta, g.eps = ctypes.c_void_p(norm.weight.data_ptr()), ctypes.c_void_p(norm.bias.data_ptr()), float(norm.eps)
        keep += [norm.weight, norm.bias]
    if post is not None:
        t, g.post, g.ld_post = _rows2d(post, "post")
        keep.append(t)
    if x_out is not None:
        t, g.x_out, g.ld_xout = _rows2d(x_out, "x_out")
        keep.append(t)
    if split_out is not None:
        g.split_out, g.split_scale = ctypes.c_void_p(split_out.data_ptr()), SPLIT_ACT_SCALE
        g.split_pad, g.split_layout = (0, 1) if split_lines else (SPLIT_BIAS_PAD, 0)
        keep.append(split_out)
    g._keep, g._held = keep, held
    return g


def row_gemm(segs, weight, bias, out, relu_from=None):
    """out = [relu on columns >= relu_from](cat(segs) @ weight.T + bias); weight [N, 256*len(segs)] contiguous.
    Like row_seg's, the description is for rowgemm_launch only, which checks the row counts and that every tensor is on the GPU."""
    if weight.dim() != 2 or weight.shape[1] != 256 * len(segs) or not weight.is_contiguous() or weight.dtype != torch.float32:
        raise RuntimeError("row_gemm: weight must be a contiguous float32 [N, 256 * segments] tensor")
    N, K = weight.shape
    _sized("row_gemm", "bias", bias, N, f"N = {N}")
    if out.dim() not in (2, 3) or out.shape[-1] != N:
        raise RuntimeError(f"row_gemm: out must be [rows, N = {N}], got {tuple(out.shape)}")
    d = _lib.RowGemm()
    for i, g in enumerate(segs):
        d.seg[i] = g
    d.num_seg, d.N = len(segs), N
    d.w = ctypes.c_void_p(weight.data_ptr())
    d.b = ctypes.c_void_p(bias.data_ptr()) if bias is not None else None
    t, d.out, d.ld_out = _rows2d(out, "out")
    d.relu_from = N if relu_from is None else int(relu_from)
    d._keep = [segs, weight, bias, t]
    d._out_rows = int(torch.Size(out.shape[:-1]).numel())
    return d


def rowgemm_launch(descs, rows):
    """One launch for up to 3 independent row GEMMs over the same rows.  Refuses a launch whose kernel would read or write
    past an operand: every operand of every segment, and ``out``, holds at least ``rows`` rows (their widths were checked
    when the segments were described)."""
    rows = int(rows)
    for i, d in enumerate(descs):
        segs, weight, bias, out = d._keep
        for s, g in enumerate(segs):
            for name, held in g._held.items():
                if held < rows:
                    raise RuntimeError(f"rowgemm_launch: GEMM {i} segment {s}: {name} holds {held} rows, the launch covers {rows}")
        if d._out_rows < rows:
            raise RuntimeError(f"rowgemm_launch: GEMM {i}: out holds {d._out_rows} rows, the launch covers {rows}")
    for i, d in enumerate(descs):
        segs, weight, bias, out = d._keep
        tensors = [weight, out] + ([bias] if bias is not None else []) + [t for g in segs for t in g._keep]
        if not all(t.is_cuda for t in tensors):
            raise RuntimeError(f"racformer_amd.rowgemm_launch: GEMM {i}: every operand must be a CUDA tensor (HIP device); "
                               "the hot path has no CPU fallback")
    arr = (_lib.RowGemm * len(descs))(*descs)
    rc = _lib.lib().rac_rowgemm_fwd(arr, len(descs), rows, _lib.stream_ptr())
    _lib.check(rc, "rac_rowgemm_fwd")


# ------------------------------------------------------------------------------------------- split-precision GEMM
def pack_gemm_split_weight(weight):
    """nn.Linear weight [N, K] fp32 (device) -> (f16 line image [N, K/32, 64] = [hi 32 | lo 32] of weight * 2^s, alpha) for
    rac_outproj_fwd: alpha = 2^-s / SPLIT_ACT_SCALE undoes the weight's and the activation image's power-of-two scalings.
    (None, None) if f16 cannot hold the weights or K is not a multiple of 32."""
    import math
    w = weight.detach().float().contiguous()
    N, K = w.shape
    amax = float(w.abs().max())
    if K % 32 != 0 or not w.is_cuda or not (amax > 0.0) or amax != amax or amax == float("inf"):
        return None, None
    s = 13 - math.frexp(amax)[1] + 1          # amax * 2^s in [2^13, 2^14)
    img = torch.empty(N, K // 32, 64, device=w.device, dtype=torch.float16)
    _lib.check(_lib.lib().rac_gemm_split_pack_fwd(_lib.ptr(w), _lib.ptr(img), N, K, float(2.0 ** s), _lib.stream_ptr()),
               "rac_gemm_split_pack_fwd")
    return img, 2.0 ** (-s) / SPLIT_ACT_SCALE


def value_proj_fused(maps, w_image, w_alpha, add=None, bias=None, q16=False):
    """maps f32 [F, 256, H, W] (channel-first BEV maps), w_image f16 [256, 8, 64] (pack_gemm_split_weight), w_alpha = 2^-s of the
    image, add f32 [H*W, 256] (frame-independent term) or bias [256] -> f32 [F, H*W, 256] = maps^T @ W^T + add (rac_value_proj_fwd);
    with ``q16`` the same result in the int16 block storage of quantize_values_i16: (q int16 [F, H*W, 4, 64], scale f32 [F, H*W, 4]),
    quantised in the kernel's epilogue (rac_value_proj_q16_fwd)."""
    _lib.require_gpu(maps, w_image, what="value_proj_fused")
    F_, C, H, W = maps.shape
    if maps.dtype != torch.float32 or not maps.is_contiguous() or w_image.dtype != torch.float16 or tuple(w_image.shape) != (256, 8, 64):
        raise RuntimeError("value_proj_fused: maps must be contiguous float32 [F,256,H,W], w_image f16 [256,8,64]")
    if add is not None and (add.dtype != torch.float32 or not add.is_contiguous() or tuple(add.shape) != (H * W, 256)):
        raise RuntimeError("value_proj_fused: add must be a contiguous float32 [H*W, 256] tensor")
    if q16:
        out = torch.empty(F_, H * W, 4, 64, device=maps.device, dtype=torch.int16)
        scale = torch.empty(F_, H * W, 4, device=maps.device, dtype=torch.float32)
    else:
        out = torch.empty(F_, H * W, 256, device=maps.device, dtype=torch.float32)
    ev = _lib.timer.record("value_proj_fwd") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    head = (_lib.ptr(maps), _lib.ptr(w_image), float(w_alpha), _lib.ptr(add) if add is not None else None,
            _lib.ptr(bias) if bias is not None else None)
    tail = (F_, C, H * W, 256, _lib.stream_ptr())
    if q16:
        rc, what = _lib.lib().rac_value_proj_q16_fwd(*head, _lib.ptr(out), _lib.ptr(scale), *tail), "rac_value_proj_q16_fwd"
    else:
        rc, what = _lib.lib().rac_value_proj_fwd(*head, _lib.ptr(out), *tail), "rac_value_proj_fwd"
    if ev:
        ev[1].record()
    _lib.check(rc, what)
    return (out, scale) if q16 else out


def generator_fused(x_image, w_image, bias, alpha, timer_name="mixing_generator_gemm", ld_out=None):
    """x_image f16 [M, K/32 * 64] (row_seg(split_lines=True) / add_ln(split_lines=True)), w_image f16 [N, K/32, 64] -> fp32 [M, N] =
    alpha * X @ W^T + bias (rac_generator_fwd), one launch."""
    _lib.require_gpu(x_image, w_image, what="generator_fused")
    M = x_image.shape[0]
    N, lines, _ = w_image.shape
    if x_image.dtype != torch.float16 or w_image.dtype != torch.float16 or x_image.numel() != M * lines * 64 or w_image.shape[2] != 64:
        raise RuntimeError("generator_fused: operand images do not match")
    ld_out = N if ld_out is None else int(ld_out)     # (row stride: a multiple of 4, >= N; the result has ld_out columns)
    out = torch.empty(M, ld_out, device=x_image.device, dtype=torch.float32)
    ev = _lib.timer.record(timer_name) if _lib.timer is not None and timer_name else None
    if ev:
        ev[0].record()
    rc = _lib.lib().rac_generator_fwd(_lib.ptr(x_image), _lib.ptr(w_image), _lib.ptr(bias) if bias is not None else None, float(alpha),
                                      _lib.ptr(out), ld_out, M, N, lines * 32, _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_generator_fwd")
    return out


def outproj_fused(z_image, w_image, slices):
    """z_image f16 [M, K/32, 64], w_image f16 [N, K/32, 64] -> fp32 partials [slices, M, N] (unscaled), one launch."""
    _lib.require_gpu(z_image, w_image, what="outproj_fused")
    M, lines, _ = z_image.shape
    N = w_image.shape[0]
    if z_image.dtype != torch.float16 or w_image.dtype != torch.float16 or tuple(w_image.shape[1:]) != (lines, 64) \
            or z_image.shape[2] != 64 or lines % slices != 0:
        raise RuntimeError("outproj_fused: operand images do not match")
    out = torch.empty(slices, M, N, device=z_image.device, dtype=torch.float32)
    ev = _lib.timer.record("mixing_out_proj_gemm") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    rc = _lib.lib().rac_outproj_fwd(_lib.ptr(z_image), _lib.ptr(w_image), _lib.ptr(out), M, N, lines * 32, slices, _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_outproj_fwd")
    return out


# ------------------------------------------------------------------------------------------- the mixing Linears under autograd
def _f32_rows(t, what, width=None):
    """2-D float32 CUDA rows with unit inner stride, a row stride that is a multiple of 4 and a 16-byte aligned start ->
    (pointer, M, width, row stride).  There is no CPU fallback."""
    if not t.is_cuda:
        raise RuntimeError(f"racformer_amd.{what}: tensor must be a CUDA tensor (HIP device); the hot path has no CPU fallback")
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] < 1 or (width is not None and t.shape[1] != width):
        raise RuntimeError(f"racformer_amd.{what}: expected float32 rows [M, {width if width is not None else 'K'}], M >= 1")
    ld = int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))
    if t.stride(1) != 1 or ld < t.shape[1] or ld % 4 != 0 or t.data_ptr() % 16 != 0:
        raise RuntimeError(f"racformer_amd.{what}: rows need unit inner stride, a row stride >= the width that is a multiple of 4 "
                           "and a 16-byte aligned start")
    return _lib.ptr(t), int(t.shape[0]), int(t.shape[1]), ld


def _amax1(amax, what):
    if not amax.is_cuda:
        raise RuntimeError(f"racformer_amd.{what}: amax must be a CUDA tensor (HIP device); the hot path has no CPU fallback")
    if amax.dtype != torch.float32 or amax.numel() != 1:
        raise RuntimeError(f"racformer_amd.{what}: amax must be one float32 (absmax_device)")
    return _lib.ptr(amax)


def absmax_device(*tensors, floor=0.0):
    """max(floor, max |v|) over contiguous float32 CUDA tensors -> float32 [1] ON THE DEVICE (rac_absmax_fwd): the scale source of
    linear_pack_act and linear_wgrad, never read by the host."""
    _lib.require_gpu(*tensors, what="absmax_device")
    if not tensors or any(t.dtype != torch.float32 for t in tensors):
        raise RuntimeError("absmax_device: float32 tensors expected")
    n = len(tensors)
    amax = torch.empty(1, device=tensors[0].device, dtype=torch.float32)
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in tensors])
    counts = (ctypes.c_int64 * n)(*[t.numel() for t in tensors])
    _lib.check(_lib.lib().rac_absmax_fwd(ptrs, counts, n, float(floor), _lib.ptr(amax), _lib.stream_ptr()), "rac_absmax_fwd")
    return amax


def linear_pack_act(src, amax, out=None):
    """src float32 rows [M, K] (K % 32 == 0; a row stride of its own is allowed), amax float32 [1] on the device (absmax_device over
    the same values) -> f16 line image [M, K/32, 64] = [hi 32 | lo 32] of src * rac_act_scale(amax) (rac_linear_pack_act): the X / Z
    operand of generator_ds / outproj_fused and the narrow operand of linear_wgrad."""
    p_src, M, K, ld = _f32_rows(src, "linear_pack_act")
    p_amax = _amax1(amax, "linear_pack_act")
    if K % 32 != 0:
        raise RuntimeError(f"linear_pack_act: K = {K} must be a multiple of 32")
    if out is None:
        out = torch.empty(M, K // 32, 64, device=src.device, dtype=torch.float16)
    elif tuple(out.shape) != (M, K // 32, 64) or out.dtype != torch.float16 or not out.is_contiguous() or not out.is_cuda:
        raise RuntimeError(f"linear_pack_act: out must be a contiguous CUDA float16 tensor of shape {(M, K // 32, 64)}")
    ev = _lib.timer.record("linear_pack_act") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    rc = _lib.lib().rac_linear_pack_act(p_src, ld, p_amax, _lib.ptr(out), M, K, _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_linear_pack_act")
    return out


def pack_linear_weight_t(weight):
    """nn.Linear weight [N, K] fp32 (device, N and K multiples of 32) -> (f16 line image [K, N/32, 64] of weight^T * 2^s, 2^-s)
    (rac_linear_pack_wt), the scale as pack_gemm_split_weight computes it (one host read: pack once per weight version).
    (None, None) if f16 cannot hold the weights (all zero, non-finite) or a side is not a multiple of 32."""
    import math
    if not weight.is_cuda:
        raise RuntimeError("racformer_amd.pack_linear_weight_t: tensor must be a CUDA tensor (HIP device); the hot path has no CPU fallback")
    w = weight.detach().float().contiguous()
    if w.dim() != 2:
        raise RuntimeError("pack_linear_weight_t: a 2-D weight expected")
    N, K = w.shape
    amax = float(w.abs().max())
    if K % 32 != 0 or N % 32 != 0 or not (amax > 0.0) or amax != amax or amax == float("inf"):
        return None, None
    s = 13 - math.frexp(amax)[1] + 1          # amax * 2^s in [2^13, 2^14)
    img = torch.empty(K, N // 32, 64, device=w.device, dtype=torch.float16)
    _lib.check(_lib.lib().rac_linear_pack_wt(_lib.ptr(w), _lib.ptr(img), N, K, float(2.0 ** s), _lib.stream_ptr()), "rac_linear_pack_wt")
    return img, 2.0 ** (-s)


def generator_ds(x_image, w_image, bias, alpha, amax, out=None):
    """x_image f16 [M, 8, 64] (linear_pack_act with ``amax``), w_image f16 [N, 8, 64] -> fp32 [M, N] =
    alpha / rac_act_scale(amax) * X @ W^T + bias (rac_generator_ds_fwd: rac_generator_fwd's K == 256 kernel reading the activation
    scale on the device).  ``out``: destination rows [M, N] (a row stride of its own is allowed)."""
    _lib.require_gpu(x_image, w_image, what="generator_ds")
    p_amax = _amax1(amax, "generator_ds")
    M, N = x_image.shape[0], w_image.shape[0]
    if x_image.dtype != torch.float16 or w_image.dtype != torch.float16 or tuple(x_image.shape[1:]) != (8, 64) \
            or tuple(w_image.shape[1:]) != (8, 64) or M < 1:
        raise RuntimeError("generator_ds: operand images must be float16 [M, 8, 64] and [N, 8, 64] (K = 256)")
    if bias is not None and (not bias.is_cuda or bias.dtype != torch.float32 or bias.numel() != N or not bias.is_contiguous()):
        raise RuntimeError(f"generator_ds: bias must be a contiguous float32 CUDA [{N}] tensor")
    if out is None:
        out = torch.empty(M, (N + 3) // 4 * 4, device=x_image.device, dtype=torch.float32)[:, :N]
    p_out, Mo, _, ld = _f32_rows(out, "generator_ds(out)", N)
    if Mo != M:
        raise RuntimeError(f"generator_ds: out must have {M} rows")
    ev = _lib.timer.record("generator_ds") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    rc = _lib.lib().rac_generator_ds_fwd(_lib.ptr(x_image), _lib.ptr(w_image), _lib.ptr(bias) if bias is not None else None, float(alpha),
                                         p_amax, p_out, ld, M, N, 256, _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_generator_ds_fwd")
    return out


def linear_reduce(partials, bias, amax, alpha, out=None):
    """partials f32 [slices, M, N] (outproj_fused) -> f32 [M, N] = bias + alpha / rac_act_scale(amax) * (the slices added in
    ascending order) (rac_linear_reduce).  ``out``: destination rows [M, N] (a row stride of its own is allowed)."""
    _lib.require_gpu(partials, what="linear_reduce")
    p_amax = _amax1(amax, "linear_reduce")
    if partials.dtype != torch.float32 or partials.dim() != 3 or partials.shape[2] % 4 != 0 or partials.shape[1] < 1:
        raise RuntimeError("linear_reduce: partials must be float32 [slices, M, N] with N a multiple of 4")
    S, M, N = partials.shape
    if bias is not None and (not bias.is_cuda or bias.dtype != torch.float32 or bias.numel() != N or not bias.is_contiguous()):
        raise RuntimeError(f"linear_reduce: bias must be a contiguous float32 CUDA [{N}] tensor")
    if out is None:
        out = torch.empty(M, N, device=partials.device, dtype=torch.float32)
    p_out, Mo, _, ld = _f32_rows(out, "linear_reduce(out)", N)
    if Mo != M:
        raise RuntimeError(f"linear_reduce: out must have {M} rows")
    _lib.check(_lib.lib().rac_linear_reduce(_lib.ptr(partials), _lib.ptr(bias) if bias is not None else None, p_amax, float(alpha),
                                            p_out, ld, S, M, N, _lib.stream_ptr()), "rac_linear_reduce")
    return out


def outproj_slices(K):
    """Split-K factor of rac_outproj_fwd for a reduction of length K: about 1024 per slice, a divisor of K / 32."""
    lines = K // 32
    s = max(1, lines // 32)
    while lines % s != 0:
        s -= 1
    return s


def linear_wgrad(narrow_image, amax_narrow, wide, amax_wide, wide_major, colsum=False, out=None):
    """C[a][b] = sum_m A[m][a] * Bm[m][b] (rac_linear_wgrad): ``narrow_image`` f16 [M, 8, 64] = linear_pack_act(A [M, 256],
    amax_narrow); ``wide`` float32 rows [M, Wd] (Wd a multiple of 128; a row stride of its own is allowed) with ``amax_wide`` =
    absmax_device over it.  -> f32 [256, Wd], or with ``wide_major`` [Wd, 256]; with ``colsum`` also f32 [Wd] = sum_m Bm[m][b]
    (returned as a pair).  All rows are walked in ascending order by one workgroup per 128 columns: bitwise reproducible.
    ``out``: a contiguous destination of the result's shape."""
    _lib.require_gpu(narrow_image, what="linear_wgrad")
    p_wide, M, Wd, ld = _f32_rows(wide, "linear_wgrad(wide)")
    p_an, p_aw = _amax1(amax_narrow, "linear_wgrad"), _amax1(amax_wide, "linear_wgrad")
    if narrow_image.dtype != torch.float16 or tuple(narrow_image.shape) != (M, 8, 64):
        raise RuntimeError(f"linear_wgrad: narrow_image must be float16 [{M}, 8, 64] (the narrow side is 256)")
    if Wd % 128 != 0:
        raise RuntimeError(f"linear_wgrad: the wide side {Wd} must be a multiple of 128")
    shape = (Wd, 256) if wide_major else (256, Wd)
    if out is None:
        out = torch.empty(shape, device=wide.device, dtype=torch.float32)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise RuntimeError(f"linear_wgrad: out must be a contiguous CUDA float32 tensor of shape {shape}")
    cs = torch.empty(Wd, device=wide.device, dtype=torch.float32) if colsum else None
    ev = _lib.timer.record("linear_wgrad") if _lib.timer is not None else None
    if ev:
        ev[0].record()
    rc = _lib.lib().rac_linear_wgrad(_lib.ptr(narrow_image), p_an, p_wide, ld, p_aw, _lib.ptr(out), _lib.ptr(cs) if colsum else None,
                                     M, 256, Wd, 1 if wide_major else 0, _lib.stream_ptr())
    if ev:
        ev[1].record()
    _lib.check(rc, "rac_linear_wgrad")
    return (out, cs) if colsum else out


def split_generator_forward(query, packs, bias):
    """parameter_generator on the training route: query f32 [M, 256] -> (params f32 [M, N], amax of the query on the device)."""
    amax = absmax_device(query)
    img = linear_pack_act(query, amax)
    return generator_ds(img, packs["gen_img"], bias, packs["gen_alpha"], amax), amax


def split_generator_backward(query, amax_q, grad_params, packs, need_query, need_w, need_b):
    """Gradients of split_generator_forward: grad_params f32 [M, N] contiguous -> (grad_query [M, 256], grad_weight [N, 256],
    grad_bias [N]; None where not asked for).  The data gradient is rac_outproj_fwd's split-K kernel on the image of grad_params
    and the transposed weight image (slices added in ascending order by rac_linear_reduce); the weight gradient rac_linear_wgrad
    reading grad_params as fp32, with the bias gradient from the same pass."""
    gq = gw = gb = None
    if not (need_query or need_w or need_b):
        return gq, gw, gb
    M, N = grad_params.shape
    amax_g = absmax_device(grad_params) if need_query or need_w else None
    if need_query:
        wt = packs.transposed("gen")
        if wt[0] is None:       # (an all-zero weight has no power-of-two scale to pack with: its data gradient is exactly zero)
            gq = torch.zeros_like(query)
        else:
            g_img = linear_pack_act(grad_params, amax_g)
            gq = linear_reduce(outproj_fused(g_img, wt[0], outproj_slices(N)), None, amax_g, wt[1])
            del g_img
    if need_w:
        q_img = linear_pack_act(query, amax_q)
        res = linear_wgrad(q_img, amax_q, grad_params, amax_g, True, colsum=need_b)
        gw, gb = res if need_b else (res, None)
    elif need_b:
        gb = grad_params.sum(0)
    return gq, gw, gb


def split_outproj_forward(z, packs, bias):
    """out_proj on the training route: z f32 [M, K] -> (f32 [M, 256] = z W^T + bias, amax of z on the device)."""
    amax = absmax_device(z)
    img = linear_pack_act(z, amax)
    K = z.shape[1]
    return linear_reduce(outproj_fused(img, packs["out_img"], outproj_slices(K)), bias, amax, packs["out_alpha"]), amax


def split_outproj_backward(z, amax_z, grad_out, packs, need_z, need_w, need_b):
    """Gradients of split_outproj_forward: grad_out f32 [M, 256] contiguous -> (grad_z [M, K], grad_weight [256, K], grad_bias
    [256]; None where not asked for).  The data gradient is rac_generator_fwd's K == 256 kernel on the image of grad_out and the
    transposed weight image; the weight gradient rac_linear_wgrad reading z as fp32; the bias gradient a torch sum."""
    gz = gw = None
    gb = grad_out.sum(0) if need_b else None       # (torch's reduction: a fixed tree, no atomics)
    if need_z or need_w:
        amax_g = absmax_device(grad_out)
        g_img = linear_pack_act(grad_out, amax_g)
        if need_z:
            wt = packs.transposed("out")
            gz = generator_ds(g_img, wt[0], None, wt[1], amax_g) if wt[0] is not None else torch.zeros_like(z)
        if need_w:
            gw = linear_wgrad(g_img, amax_g, z, amax_z, False)
    return gz, gw, gb


class LinearGradPacks(dict):
    """The weight images of the training route's two Linears for ONE version of the weights: "gen_img" / "gen_alpha" and
    "out_img" / "out_alpha" (pack_gemm_split_weight; alpha = 2^-s, without an activation factor: the activations' scale lives on
    the device), and -- packed on first use by a backward -- the transposed images ``transposed("gen" | "out")``."""

    def __init__(self, gen_weight, out_weight):
        super().__init__()
        self._w = dict(gen=gen_weight, out=out_weight)
        self._t = {}
        for name, w in self._w.items():
            img, alpha = pack_gemm_split_weight(w)
            if img is None:
                return
            self[name + "_img"], self[name + "_alpha"] = img, alpha * SPLIT_ACT_SCALE

    def complete(self):
        return "gen_img" in self and "out_img" in self

    def transposed(self, name):
        hit = self._t.get(name)
        if hit is None:
            hit = self._t[name] = pack_linear_weight_t(self._w[name])
        return hit


# ------------------------------------------------------------------------------------------- decode
def decode_fused(cls_scores, bbox_preds, max_num, post_center_range, score_threshold=None, out=None):
    """NMSFreeCoder.decode_single + get_bboxes' reshuffle for one sample in one launch (rac_decode_fwd):
    cls_scores [Q,C] logits, bbox_preds [Q,10] -> [max_num, 11] = (x, y, z_bottom, w, l, h, yaw, vx, vy, score, label),
    score = -1 on rows that fail the centre-range / score masks."""
    cls_scores, bbox_preds = cls_scores.contiguous(), bbox_preds.contiguous()
    _lib.require_gpu(cls_scores, bbox_preds, what="decode_fused")
    Q, C = cls_scores.shape
    if out is None:
        out = torch.empty(max_num, 11, device=cls_scores.device, dtype=torch.float32)
    rng = (ctypes.c_float * 6)(*[float(v) for v in post_center_range])
    rc = _lib.lib().rac_decode_fwd(_lib.ptr(cls_scores), _lib.ptr(bbox_preds), _lib.ptr(out), Q, C, int(max_num), rng,
                                   float(score_threshold or 0.0), int(bool(score_threshold)), _lib.stream_ptr())
    _lib.check(rc, "rac_decode_fwd")
    return out



# ------------------------------------------------------------------------------------------- head loss
def _gt_offsets(counts, what):
    off = [0]
    for n in counts:
        off.append(off[-1] + int(n))
    if len(counts) > 64:
        raise RuntimeError(f"racformer_amd.{what}: at most 64 samples a call")
    return off, (ctypes.c_int32 * len(off))(*off)


def _f32_gpu(what, *tensors):
    _lib.require_gpu(*tensors, what=what)
    for t in tensors:
        if t.dtype != torch.float32:
            raise RuntimeError(f"racformer_amd.{what}: float32 tensors only")


def match_cost_fused(all_cls_scores, all_bbox_preds, gt_boxes, gt_labels, counts, code_weights, cls_weight, reg_weight,
                     theta_weight=None, out=None):
    """The assigners' cost matrices of every (layer, sample) in one launch (rac_match_cost_fwd).  all_cls_scores [L,B,Q,C],
    all_bbox_preds [L,B,Q,10] (detached); gt_boxes [sum G, 9], gt_labels [sum G] int32: the samples' ground truth concatenated;
    counts: the host list of boxes per sample; theta_weight None: no ThetaL1Cost (HungarianAssigner3D).
    -> cost [L*B, Gmax, Qpad] (Qpad: Q rounded up to 64); entries beyond a sample's boxes or beyond Q are not written."""
    _f32_gpu("match_cost_fused", all_cls_scores, all_bbox_preds, gt_boxes, code_weights)
    _lib.require_gpu(gt_labels, what="match_cost_fused")
    if gt_labels.dtype != torch.int32:
        raise RuntimeError("racformer_amd.match_cost_fused: gt_labels must be int32")
    L, B, Q, C = all_cls_scores.shape
    off, c_off = _gt_offsets(counts, "match_cost_fused")
    if len(counts) != B or off[-1] != gt_boxes.shape[0] or gt_labels.shape[0] != off[-1] or tuple(all_bbox_preds.shape) != (L, B, Q, 10) \
            or gt_boxes.shape[-1] != 9 or code_weights.numel() != 10:
        raise RuntimeError("racformer_amd.match_cost_fused: shapes do not fit (boxes [L,B,Q,10], ground truth [sum G,9], one count per sample)")
    gmax, qpad = max(counts) if counts else 0, (Q + 63) // 64 * 64
    if out is None:
        out = torch.empty(L * B, gmax, qpad, device=all_cls_scores.device, dtype=torch.float32)
    elif tuple(out.shape) != (L * B, gmax, qpad) or out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError("racformer_amd.match_cost_fused: out must be a contiguous float32 [L*B, Gmax, Qpad]")
    rc = _lib.lib().rac_match_cost_fwd(_lib.ptr(all_cls_scores), _lib.ptr(all_bbox_preds), _lib.ptr(gt_boxes), _lib.ptr(gt_labels), c_off,
                                       _lib.ptr(code_weights), _lib.ptr(out), L, B, Q, C, gmax, qpad, float(cls_weight), float(reg_weight),
                                       float(theta_weight or 0.0), int(theta_weight is not None), _lib.stream_ptr())
    _lib.check(rc, "rac_match_cost_fwd")
    return out


def lsap_fused(cost, counts, num_layers, num_query, with_steps=False):
    """The L*B assignment problems of a match_cost_fused tensor on the device (rac_lsap_fwd): no host read-back.
    -> matched_query [P,Gmax] int32, assigned_gt [P,Q] int32 (index into the concatenated ground truth, -1 background),
    u [P,Gmax] and v [P,Q] float64 duals (, steps [P] int32)."""
    _f32_gpu("lsap_fused", cost)
    P, gmax, qpad = cost.shape
    B = len(counts)
    _, c_off = _gt_offsets(counts, "lsap_fused")
    if P != num_layers * B or gmax != (max(counts) if counts else 0) or qpad < num_query:
        raise RuntimeError("racformer_amd.lsap_fused: cost must be [num_layers * len(counts), max(counts), >= num_query]")
    dev = cost.device
    matched = torch.empty(P, gmax, device=dev, dtype=torch.int32)
    assigned = torch.empty(P, num_query, device=dev, dtype=torch.int32)
    u = torch.empty(P, gmax, device=dev, dtype=torch.float64)
    v = torch.empty(P, num_query, device=dev, dtype=torch.float64)
    steps = torch.empty(P, device=dev, dtype=torch.int32) if with_steps else None
    rc = _lib.lib().rac_lsap_fwd(_lib.ptr(cost), c_off, _lib.ptr(matched), _lib.ptr(assigned), _lib.ptr(u), _lib.ptr(v),
                                 _lib.ptr(steps) if with_steps else None, num_layers, B, num_query, gmax, qpad, _lib.stream_ptr())
    _lib.check(rc, "rac_lsap_fwd")
    return (matched, assigned, u, v, steps) if with_steps else (matched, assigned, u, v)


def det_loss_fused(logits, boxes, target, gt_boxes, gt_labels, code_weights, alpha=0.25, gamma=2.0):
    """Focal + L1 sums of rows [L,R] with their unit gradients in one launch (rac_det_loss_fwd).  logits [L,R,C], boxes [L,R,10];
    target [L,R] int32 (index into gt_boxes / gt_labels, -1 background) or None (row r takes entry r mod len(gt_boxes)).
    -> sums [L,2], grad_logits [L,R,C], grad_boxes [L,R,10]."""
    _f32_gpu("det_loss_fused", logits, boxes, gt_boxes, code_weights)
    L, R, C = logits.shape
    if tuple(boxes.shape) != (L, R, 10) or gt_boxes.shape[-1] != 9 or gt_labels.shape[0] != gt_boxes.shape[0] or code_weights.numel() != 10:
        raise RuntimeError("racformer_amd.det_loss_fused: shapes do not fit (boxes [L,R,10], ground truth [n,9] with n labels)")
    for t in (gt_labels, target):
        if t is not None:
            _lib.require_gpu(t, what="det_loss_fused")
            if t.dtype != torch.int32:
                raise RuntimeError("racformer_amd.det_loss_fused: gt_labels and target must be int32")
    if target is not None and tuple(target.shape) != (L, R):
        raise RuntimeError("racformer_amd.det_loss_fused: target must be [L,R]")
    sums = torch.empty(L, 2, device=logits.device, dtype=torch.float32)
    g_logits, g_boxes = torch.empty_like(logits), torch.empty_like(boxes)
    rc = _lib.lib().rac_det_loss_fwd(_lib.ptr(logits), _lib.ptr(boxes), _lib.ptr(target) if target is not None else None, _lib.ptr(gt_boxes),
                                     _lib.ptr(gt_labels), _lib.ptr(code_weights), _lib.ptr(sums), _lib.ptr(g_logits), _lib.ptr(g_boxes),
                                     L, R, C, gt_boxes.shape[0], float(alpha), float(gamma), _lib.stream_ptr())
    _lib.check(rc, "rac_det_loss_fwd")
    return sums, g_logits, g_boxes


def lsap_host(cost_gq=None, cost_qg=None):
    """One assignment problem on the host (rac_lsap_host, plain C++ in float64; no GPU, no scipy).  Give the float32 cost as
    cost_gq [G,Q] or as cost_qg [Q,G] (the reference's layout), any strides, CPU memory.
    -> matched_query [G] int32 (-1: unmatched), matched_gt [Q] int32 (-1: background), u [G], v [Q] float64, steps."""
    c = cost_gq if cost_gq is not None else cost_qg
    if c.is_cuda or c.dtype != torch.float32 or c.dim() != 2:
        raise RuntimeError("racformer_amd.lsap_host: a float32 CPU matrix")
    (G, Q), (gs, qs) = (c.shape, c.stride()) if cost_gq is not None else (c.shape[::-1], c.stride()[::-1])
    mq, mg = torch.empty(G, dtype=torch.int32), torch.empty(Q, dtype=torch.int32)
    u, v = torch.empty(G, dtype=torch.float64), torch.empty(Q, dtype=torch.float64)
    steps = ctypes.c_int64(0)
    rc = _lib.lib().rac_lsap_host(_lib.ptr(c), gs, qs, G, Q, _lib.ptr(mq), _lib.ptr(mg), _lib.ptr(u), _lib.ptr(v),
                                  ctypes.cast(ctypes.pointer(steps), ctypes.c_void_p))
    _lib.check(rc, "rac_lsap_host")
    return mq, mg, u, v, steps.value


# ------------------------------------------------------------------------------------------- streaming frame memory
def frames_gather(rings, outs, slots):
    """The streaming detector's window from its frame memory in one launch (rac_frames_gather): for every pair
    (``rings[k]`` [n_slots, *frame], ``outs[k]`` whose leading dimensions hold ``len(slots)`` frames of that shape) and every t,
    frame t of ``outs[k]`` = frame ``slots[t]`` of ``rings[k]``.  Contiguous device tensors, a frame a multiple of 16 bytes; up to 8
    tensors and 16 frames.  ``slots``: host integers -- they travel as kernel arguments, nothing is uploaded."""
    rings, outs, slots = list(rings), list(outs), [int(s) for s in slots]
    if len(rings) != len(outs) or not rings:
        raise RuntimeError("frames_gather: one out per ring, at least one")
    _lib.require_gpu(*rings, *outs, what="frames_gather")
    n_slots, T = int(rings[0].shape[0]), len(slots)
    fb = []
    for r, o in zip(rings, outs):
        frame = r[0].numel() * r.element_size() if r.shape[0] else 0
        if r.shape[0] != n_slots or r.dtype != o.dtype or o.numel() * o.element_size() != T * frame:
            raise RuntimeError("frames_gather: every ring holds n_slots frames and every out len(slots) frames of its ring's dtype and size")
        fb.append(frame)
    n = len(rings)
    rc = _lib.lib().rac_frames_gather(n, (ctypes.c_void_p * n)(*[r.data_ptr() for r in rings]), (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]),
                                      (ctypes.c_int64 * n)(*fb), (ctypes.c_int32 * max(T, 1))(*slots), T, n_slots, _lib.stream_ptr())
    _lib.check(rc, "rac_frames_gather")
    return outs
