"""Host side of the temporal-fusion convolution's backward: the transposed, flipped weight packer of the data gradient and the
argument checks of the new C entry points (no GPU)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from racformer_amd import _lib
from racformer_amd.fused import (conv3x3_dgrad_weight, pack_conv3x3_dgrad_weight, pack_conv3x3_weight, unpack_conv3x3_weight,
                                 wgrad_k_splits)


def _weight(cin, cout=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(cout, cin, 3, 3, generator=g) * 0.05).float()


def test_dgrad_weight_is_autograds_input_gradient():
    """F.conv2d(dY, W', padding=1) in float64 equals autograd's input gradient of F.conv2d(X, W, padding=1)."""
    g = torch.Generator().manual_seed(1)
    w = torch.randn(8, 6, 3, 3, generator=g, dtype=torch.float64)
    x = torch.randn(2, 6, 5, 7, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(2, 8, 5, 7, generator=g, dtype=torch.float64)
    F.conv2d(x, w, padding=1).backward(dy)
    wt = conv3x3_dgrad_weight(w)
    assert tuple(wt.shape) == (6, 8, 3, 3)
    got = F.conv2d(dy, wt, padding=1)
    assert torch.allclose(got, x.grad, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("cin,c0,rows", [(320, 0, 256), (320, 256, 64), (288, 256, 32)])
def test_packed_dgrad_image_unpacks_to_the_transposed_weights(cin, c0, rows):
    """hi + lo of the packed image give W' back to 2^-22 relative; input channels past the weights' own are zero columns."""
    w = _weight(cin, seed=cin + c0)
    ws, alpha, got_rows = pack_conv3x3_dgrad_weight(w, c0)
    assert got_rows == rows and tuple(ws.shape) == (9, 8, 256, 2, 32) and ws.dtype == torch.float16
    back = unpack_conv3x3_weight(ws, alpha)                     # [256 (ci of W, padded), 256 (co of W), 3, 3]
    want = conv3x3_dgrad_weight(w)[c0:c0 + 256].double()
    assert torch.equal(back[rows:], torch.zeros_like(back[rows:]))
    err = (back[:rows] - want).abs()
    # the split keeps 22 bits of every element; an f16 lo below its subnormal step adds 2^-25 of the scaled unit
    assert bool((err <= 2.0 ** -22 * want.abs() + 2.0 ** -25 * alpha).all())
    # and the unpacker inverts the forward packer the same way
    ws_f, alpha_f = pack_conv3x3_weight(w)
    err_f = (unpack_conv3x3_weight(ws_f, alpha_f) - w.double()).abs()
    assert bool((err_f <= 2.0 ** -22 * w.double().abs() + 2.0 ** -25 * alpha_f).all())


def test_k_split_count_depends_on_the_shape_alone():
    for N, H, W, cin in [(1, 16, 16, 320), (3, 20, 16, 320), (2, 8, 12, 288), (2, 2, 128, 320), (4, 32, 32, 320), (8, 128, 128, 320)]:
        k = wgrad_k_splits(N, H, W, cin)
        per = -(-N * H // k)
        assert 1 <= k <= N * H and (k - 1) * per < N * H <= k * per          # no empty range
    assert wgrad_k_splits(4, 32, 32, 320) > 1 and wgrad_k_splits(8, 128, 128, 320) > 1


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    p = ctypes.c_void_p(256)
    # rac_conv_pack_cl_fwd(src, amax, xs, N, C, H, W, c_total, c_offset, stream)
    assert lib.rac_conv_pack_cl_fwd(None, None, None, 1, 256, 4, 4, 256, 0, None) == -1
    assert b"null pointer" in lib.rac_last_error()
    assert lib.rac_conv_pack_cl_fwd(p, p, p, 1, 48, 4, 4, 256, 0, None) == -1
    assert b"multiples of 32" in lib.rac_last_error()
    assert lib.rac_conv_pack_cl_fwd(p, p, p, 1, 256, 4, 4, 256, 32, None) == -1
    assert lib.rac_conv_pack_cl_fwd(p, p, p, 1, 256, 0, 4, 256, 0, None) == -1
    assert lib.rac_conv_pack_cl_fwd(ctypes.c_void_p(260), p, p, 1, 256, 4, 4, 256, 0, None) == -1
    assert b"16-byte aligned" in lib.rac_last_error()
    # rac_conv3x3_wgrad(xs, gs, amax_x, amax_g, workspace, dw, N, H, W, Cin, Cout, k_splits, stream)
    assert lib.rac_conv3x3_wgrad(None, None, None, None, None, None, 1, 4, 4, 320, 256, 1, None) == -1
    assert b"null pointer" in lib.rac_last_error()
    for i in range(6):
        args = [p] * 6
        args[i] = None
        assert lib.rac_conv3x3_wgrad(*args, 1, 4, 4, 320, 256, 1, None) == -1 and b"null pointer" in lib.rac_last_error()
    assert lib.rac_conv3x3_wgrad(p, p, p, p, p, p, 1, 4, 4, 300, 256, 1, None) == -1
    assert b"multiple of 32" in lib.rac_last_error()
    assert lib.rac_conv3x3_wgrad(p, p, p, p, p, p, 1, 4, 4, 320, 64, 1, None) == -1
    assert b"built for 256 output channels" in lib.rac_last_error()
    assert lib.rac_conv3x3_wgrad(p, p, p, p, p, p, 1, 4, 4, 320, 256, 0, None) == -1
    assert lib.rac_conv3x3_wgrad(p, p, p, p, p, p, 1, 4, 4, 320, 256, 5, None) == -1       # more ranges than image rows
    assert b"k_splits" in lib.rac_last_error()
    assert lib.rac_conv3x3_wgrad(p, p, p, p, p, p, 0, 4, 4, 320, 256, 1, None) == -1
    # the data gradient's launch is rac_conv3x3_fwd: its own checks hold for the transposed problem too
    assert lib.rac_conv3x3_fwd(p, p, None, None, p, 1.0, p, 1, 4, 4, 256, 64, None) == -1
    assert b"built for 256 output channels" in lib.rac_last_error()


def test_all_zero_weight_slice_packs_to_none_and_its_gradient_is_zero():
    from racformer_amd.fused import _zero_dgrad
    w = _weight(320)
    w[:, 256:] = 0
    assert pack_conv3x3_dgrad_weight(w, 256) == (None, None, 0) and pack_conv3x3_dgrad_weight(w, 0)[0] is not None
    like = torch.ones(2, 64, 4, 4)
    z = _zero_dgrad(w[:, 256:], like)
    assert z.shape == like.shape and bool((z == 0).all())
    w[0, 300, 1, 1] = float("nan")
    with pytest.raises(RuntimeError):
        _zero_dgrad(w[:, 256:], like)
