"""Float64 restatement of the SASA core under a boolean attention mask (test infrastructure, shared by
tests/test_sasa_mask_cpu.py, tests/test_sasa_mask_gpu.py and tests/test_head_dn_*.py): the masks of the tests, the masked core and
the closed-form backward rac_sasa_bwd_mask implements, float64 fakes of the two launchers that take ``mask=``, and the per-kind
reference with the magnitude sums A of sasa_ref.reference_with_scales."""
import math

import numpy as np
import torch

from oracle import restate as R
from racformer_amd.fused import PackedAttnMask
from sasa_ref import _dist, _split


# ----------------------------------------------------------------------------------- masks (True: blocked)
def dn_layout(Q, groups, single):
    """the query-denoising layout (racformer_head.py:220-232): ``groups`` groups of ``single`` denoising queries in front of
    Q - groups*single matching queries; key j is allowed for query i iff j is a matching query or j is in i's group"""
    pad = groups * single
    assert pad <= Q
    idx = torch.arange(Q)
    group = torch.where(idx < pad, idx // max(single, 1), torch.full_like(idx, -1))
    return (idx[None, :] < pad) & (group[:, None] != group[None, :])


def random_mask(Q, seed, density=0.5):
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(Q, Q, generator=g) < density
    m.fill_diagonal_(False)
    return m


def tile_mask(Q, seed, tile_density=0.5, bit_density=0.05):
    """whole 16 x 16 tiles blocked (never a diagonal tile: every row keeps allowed keys) plus scattered bits, diagonal free"""
    g = torch.Generator().manual_seed(seed)
    nt = (Q + 15) // 16
    tiles = torch.rand(nt, nt, generator=g) < tile_density
    tiles.fill_diagonal_(False)
    m = tiles.repeat_interleave(16, 0).repeat_interleave(16, 1)[:Q, :Q].clone()
    m |= torch.rand(Q, Q, generator=g) < bit_density
    m.fill_diagonal_(False)
    return m


def pack_numpy(mask, extra_words=0, garbage_seed=None):
    """numpy.packbits restatement of the mask operand: int32 [Q, ceil(Q/32) + extra_words]; ``garbage_seed``: the bits past Q
    (padding of the last word and the extra words) are random instead of zero -- the kernels must ignore them"""
    Q = mask.shape[0]
    W = (Q + 31) // 32 + extra_words
    full = np.zeros((Q, W * 32), dtype=bool)
    if garbage_seed is not None:
        full[:] = np.random.default_rng(garbage_seed).random((Q, W * 32)) < 0.7
    full[:, :Q] = mask.cpu().numpy()
    words = np.packbits(full, axis=1, bitorder="little").view(np.uint32).view(np.int32)
    return torch.from_numpy(words.copy())


def packed(mask, device, extra_words=0, garbage_seed=None):
    return PackedAttnMask(pack_numpy(mask, extra_words, garbage_seed).to(device), mask.to(device))


# ----------------------------------------------------------------------------------- the core and its backward
def _dense(mask):
    return mask.dense if isinstance(mask, PackedAttnMask) else mask


def _logits(qkv, tau, query_bbox, num_heads, pc_range, mask):
    q, k, v = _split(qkv, num_heads)
    d = q.shape[-1]
    s = (q / math.sqrt(d)) @ k.transpose(-1, -2) - _dist(query_bbox, pc_range)[:, None] * tau.double().permute(0, 2, 1)[..., None]
    if mask is not None:
        s = s.masked_fill(_dense(mask).to(s.device), -math.inf)
    return q, k, v, s


def core64(qkv, tau, query_bbox, num_heads, pc_range, mask=None):
    """-> out [B,Q,E], lse [B,heads,Q], float64 (differentiable in qkv and tau)"""
    _, _, v, s = _logits(qkv, tau, query_bbox, num_heads, pc_range, mask)
    lse = torch.logsumexp(s, dim=-1)
    o = torch.softmax(s, dim=-1) @ v
    return o.permute(0, 2, 1, 3).reshape(qkv.shape[0], qkv.shape[1], -1), lse


def closed_form_bwd(qkv, tau, query_bbox, num_heads, pc_range, out, lse, grad_out, mask=None):
    """the backward rac_sasa_bwd_mask implements, from the saved out and lse: P = exp(s - lse) on the allowed pairs, 0 elsewhere"""
    B, Q, _ = query_bbox.shape
    q, k, v, s = _logits(qkv, tau, query_bbox, num_heads, pc_range, mask)
    d = q.shape[-1]
    r = _dist(query_bbox, pc_range)[:, None]
    P = torch.exp(s - lse.double()[..., None])
    dO = grad_out.double().reshape(B, Q, num_heads, d).permute(0, 2, 1, 3)
    O = out.double().reshape(B, Q, num_heads, d).permute(0, 2, 1, 3)
    D = (dO * O).sum(-1, keepdim=True)
    dS = P * (dO @ v.transpose(-1, -2) - D)
    dq = dS @ k / math.sqrt(d)
    dk = dS.transpose(-1, -2) @ (q / math.sqrt(d))
    dv = P.transpose(-1, -2) @ dO
    dtau = -(dS * r).sum(-1)
    rows = [x.permute(0, 2, 1, 3).reshape(B, Q, -1) for x in (dq, dk, dv)]
    return torch.cat(rows, dim=-1), dtau.permute(0, 2, 1)


# float64 fakes of the two launchers (sasa_fused / sasa_backward): plain tensors in and out, no autograd history
CALLS = []


def fake_fused(qkv, tau, query_bbox, num_heads, pc_range, box_table=None, lse_out=None, mask=None):
    CALLS.append(("fwd", lse_out is not None, None if mask is None else id(mask)))
    assert mask is None or isinstance(mask, PackedAttnMask)
    with torch.no_grad():
        o, lse = core64(qkv, tau, query_bbox, num_heads, pc_range, mask)
    if lse_out is not None:
        lse_out.copy_(lse)
    return o.float()


def fake_backward(qkv, tau, query_bbox, num_heads, pc_range, out, lse, grad_out, box_table=None, grad_qkv=None, grad_tau=None,
                  mask=None):
    CALLS.append(("bwd", None, None if mask is None else id(mask)))
    with torch.no_grad():
        gq, gt = closed_form_bwd(qkv, tau, query_bbox, num_heads, pc_range, out, lse, grad_out, mask)
    grad_qkv.copy_(gq)
    grad_tau.copy_(gt)
    return grad_qkv, grad_tau


def reference_with_scales(qkv, tau, query_bbox, num_heads, pc_range, grad_out, mask):
    """sasa_ref.reference_with_scales with the mask applied: float64 backward of the masked core and, per kind, the magnitude A of
    the same computation with every term made non-negative (same sums; a blocked pair has P = 0 and carries no term; the row
    maximum of A_S is over the allowed keys, the only logits that are formed into the softmax).
    -> dict kind -> (ref, A), kinds dq, dk, dv, out [B,Q,heads*d] (out: the forward output, A as dv's), dtau [B,Q,heads], lse [B,heads,Q]."""
    B, Q, _ = query_bbox.shape
    q, k, v = _split(qkv, num_heads)
    d = q.shape[-1]
    qs = q / math.sqrt(d)
    blocked = _dense(mask).to(qkv.device)
    with torch.no_grad():
        c = R.decode_bbox(R.theta_d2xy(query_bbox.double()), pc_range)[..., :2]
    r = (c[:, :, None] - c[:, None]).norm(dim=-1)[:, None]
    cn = c.norm(dim=-1)
    csum = (cn[:, :, None] + cn[:, None])[:, None]
    ta = tau.double().permute(0, 2, 1)[..., None]
    s = (qs @ k.transpose(-1, -2) - r * ta).masked_fill(blocked, -math.inf)
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse[..., None])
    dO = grad_out.double().reshape(B, Q, num_heads, d).permute(0, 2, 1, 3)
    O = P @ v
    D = (dO * O).sum(-1, keepdim=True)
    dP = dO @ v.transpose(-1, -2)
    dS = P * (dP - D)
    AS = qs.abs() @ k.abs().transpose(-1, -2) + (r + csum) * ta.abs() + lse.abs()[..., None]
    ASmax = AS.masked_fill(blocked, 0.0).amax(-1, keepdim=True)
    AP = P * (AS + ASmax)
    AdS = AP * (dP - D).abs() + P * (dO.abs() @ v.abs().transpose(-1, -2) + (dO.abs() * O.abs()).sum(-1, keepdim=True))
    T_ = AdS + dS.abs()

    def rows(x):
        return x.permute(0, 2, 1, 3).reshape(B, Q, -1)

    return {
        "dq": (rows(dS @ k / math.sqrt(d)), rows(T_ @ k.abs() / math.sqrt(d))),
        "dk": (rows(dS.transpose(-1, -2) @ qs), rows(T_.transpose(-1, -2) @ qs.abs())),
        "dv": (rows(P.transpose(-1, -2) @ dO), rows((AP + P).transpose(-1, -2) @ dO.abs())),
        "dtau": ((-(dS * r).sum(-1)).permute(0, 2, 1), ((T_ * r).sum(-1) + (dS.abs() * csum).sum(-1)).permute(0, 2, 1)),
        "lse": (lse, (P * AS).sum(-1) + ASmax[..., 0]),
        "out": (rows(O), rows((AP + P) @ v.abs())),
    }


def freed_probability(qkv, tau, query_bbox, num_heads, pc_range, mask):
    """float64: for every blocked pair (i, j) the probability it would get in (batch 0, head 0) if that one bit were cleared:
    [Q,Q], 0 at allowed pairs.  The negative control clears the bit where this is largest."""
    q, k, _ = _split(qkv[:1], num_heads)
    d = q.shape[-1]
    r = _dist(query_bbox[:1], pc_range)[:, None]
    s = ((q / math.sqrt(d)) @ k.transpose(-1, -2) - r * tau[:1].double().permute(0, 2, 1)[..., None])[0, 0]
    blocked = _dense(mask).to(s.device)
    lse = torch.logsumexp(s.masked_fill(blocked, -math.inf), dim=-1, keepdim=True)
    p = torch.exp(s - torch.logaddexp(lse, s))
    return torch.where(blocked, p, torch.zeros_like(p))
