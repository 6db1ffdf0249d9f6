"""The image necks' backward without a GPU: the three entry points are declared, bound and exported, refuse bad arguments before any
HIP call, ``necks.nearest_children`` is the exact inverse of ``necks.nearest_src``, and the ``fused_grad`` switch routes as documented."""
import ctypes
import os
import re

import torch

from racformer_amd import _lib, necks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rac_fpn_merge_bwd", "rac_fpn_lateral_dgrad", "rac_fpn_lateral_wgrad")


def test_symbols_are_declared_bound_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "racformer_hip.h")).read(), flags=re.S)
    assert int(re.search(r"#define\s+RAC_ABI_VERSION\s+(\d+)", text).group(1)) >= 29
    kind = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_float: "f", ctypes.c_int64: "l"}
    lib = _lib.lib()
    assert lib.rac_abi_version() >= 29
    for name in NAMES:
        params = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, text)
        assert params, f"{name} is not declared in include/racformer_hip.h"
        want = ["p" if "*" in p else ("f" if p.strip().startswith("float") else "i") for p in params.group(1).split(",")]
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert [kind[a] for a in _lib.SIGNATURES[name][1]] == want, name
        assert hasattr(lib, name), f"{name} is not exported"


def _expect(call, cases, lib):
    for kw, msg in cases:
        assert call(**kw) == -1, kw
        assert msg in lib.rac_last_error(), (kw, lib.rac_last_error())


def test_merge_argument_errors_need_no_gpu():
    lib = _lib.lib()
    p16 = ctypes.c_void_p(16)

    def merge(a=p16, gfine=p16, rows=p16, cols=p16, g=p16, N=1, C=256, H=4, W=6, fh=7, fw=11):
        return lib.rac_fpn_merge_bwd(a, gfine, rows, cols, g, N, C, H, W, fh, fw, None)

    _expect(merge, [(dict(g=None), b"null pointer"), (dict(a=None, gfine=None), b"null pointer"), (dict(rows=None), b"null pointer"),
                    (dict(cols=None), b"null pointer"), (dict(H=0), b"H=0"), (dict(W=-1), b"W=-1"), (dict(C=0), b"C=0"),
                    (dict(N=-1), b"N=-1"), (dict(H=8), b"no larger than the finer one"), (dict(W=12), b"no larger than the finer one"),
                    (dict(a=ctypes.c_void_p(6)), b"4-byte aligned")], lib)
    assert merge(a=None, gfine=None, g=None, N=0) == 0


def test_dgrad_argument_errors_need_no_gpu():
    lib = _lib.lib()
    p16 = ctypes.c_void_p(16)

    def dgrad(g=p16, w=p16, dx=p16, N=1, Cin=64, H=4, W=6, Cout=256):
        return lib.rac_fpn_lateral_dgrad(g, w, 1.0, dx, N, Cin, H, W, Cout, None)

    _expect(dgrad, [(dict(g=None), b"null pointer"), (dict(w=None), b"null pointer"), (dict(dx=None), b"null pointer"),
                    (dict(Cin=48), b"multiple of 32"), (dict(Cin=0), b"multiple of 32"), (dict(Cin=4096), b"multiple of 32"),
                    (dict(Cout=128), b"256 output channels"), (dict(H=0), b"H=0"), (dict(W=0), b"W=0"), (dict(N=-2), b"N=-2"),
                    (dict(w=ctypes.c_void_p(8)), b"16-byte aligned")], lib)
    assert dgrad(g=None, w=None, dx=None, N=0) == 0


def test_wgrad_argument_errors_need_no_gpu():
    lib = _lib.lib()
    p16 = ctypes.c_void_p(16)

    def wgrad(g=p16, x=p16, work=p16, dw=p16, db=None, N=2, Cin=64, H=4, W=6, Cout=256, k=1):
        return lib.rac_fpn_lateral_wgrad(g, x, work, dw, db, N, Cin, H, W, Cout, k, None)

    _expect(wgrad, [(dict(g=None), b"null pointer"), (dict(x=None), b"null pointer"), (dict(work=None), b"null pointer"),
                    (dict(dw=None), b"null pointer"), (dict(Cin=48), b"multiple of 32"), (dict(Cin=0), b"multiple of 32"),
                    (dict(Cin=4096), b"multiple of 32"), (dict(Cout=64), b"256 output channels"), (dict(H=0), b"H=0"),
                    (dict(W=0), b"W=0"), (dict(N=0), b"N=0"), (dict(k=0), b"k_splits=0"),
                    (dict(k=3), b"k_splits=3"),                       # two units of 32 pixels (24 pixels per image, two images)
                    (dict(N=5, k=4), b"empty range"),                 # five units in ranges of two: the fourth would be empty
                    (dict(db=ctypes.c_void_p(6)), b"4-byte aligned")], lib)


def test_nearest_children_inverts_nearest_src_exhaustively():
    """For every 1 <= in <= 96 and in <= out <= 2 in + 1: the ranges [start[i], start[i + 1]) are contiguous, disjoint, cover
    0 .. out - 1, and hold exactly the fine indices whose source is i."""
    for n_in in range(1, 97):
        for n_out in range(n_in, 2 * n_in + 2):
            start = necks.nearest_children(n_in, n_out)
            assert start.dtype == torch.int32 and tuple(start.shape) == (n_in + 1,)
            s = start.tolist()
            assert s[0] == 0 and s[-1] == n_out and all(a <= b for a, b in zip(s, s[1:])), (n_in, n_out)
            src = [necks.nearest_src(d, n_in, n_out) for d in range(n_out)]
            assert src == [i for i in range(n_in) for _ in range(s[i], s[i + 1])], (n_in, n_out)


def test_wgrad_k_splits_leave_no_empty_range():
    for n, h, w, cin in [(1, 1, 1, 32), (3, 8, 22, 96), (2, 7, 11, 2048), (6, 64, 176, 32), (48, 64, 176, 256), (48, 8, 22, 2048)]:
        units = n * ((h * w + 31) // 32)
        k = necks.lateral_wgrad_k_splits(n, h, w, cin)
        per = -(-units // k)
        assert 1 <= k <= units and (k - 1) * per < units, (n, h, w, cin, k)


def test_fused_grad_is_opt_in_and_leaves_hip_route_alone():
    assert necks.FPN.fused_grad is False and necks.CustomFPN.fused_grad is False
    m = necks.FPN([32, 64], 256, 2)
    xs = [torch.zeros(2, 32, 4, 4), torch.zeros(2, 64, 2, 2)]
    assert not m.fused_grad and not m.hip_grad_route(xs)
    m.fused_grad = True
    assert not m.hip_route(xs)                  # under grad, with parameters that require it: never the no-grad route
    assert not m.hip_grad_route(xs)             # CPU tensors
    with torch.no_grad():
        assert not m.hip_grad_route(xs)
    outs = m(xs)                                # the torch route, with autograd history
    assert all(o.requires_grad for o in outs)
