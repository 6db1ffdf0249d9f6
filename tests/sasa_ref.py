"""Float64 restatement of the SASA core and of the closed-form backward rac_sasa_bwd implements (test infrastructure, shared
by tests/test_sasa_grad_cpu.py and tests/test_sasa_grad_gpu.py)."""
import math

import torch

from oracle import restate as R


def _split(qkv, num_heads):
    B, Q, W = qkv.shape
    e = W // 3
    return [x.reshape(B, Q, num_heads, e // num_heads).permute(0, 2, 1, 3).double() for x in qkv.split(e, dim=-1)]


def _dist(query_bbox, pc_range):
    with torch.no_grad():
        c = R.decode_bbox(R.theta_d2xy(query_bbox.detach().double()), pc_range)[..., :2]
        return (c[:, :, None] - c[:, None]).norm(dim=-1)                                    # [B,Q,Q]


def core64(qkv, tau, query_bbox, num_heads, pc_range):
    """-> out [B,Q,E], lse [B,heads,Q], float64 (differentiable in qkv and tau)"""
    q, k, v = _split(qkv, num_heads)
    d = q.shape[-1]
    s = (q / math.sqrt(d)) @ k.transpose(-1, -2) - _dist(query_bbox, pc_range)[:, None] * tau.double().permute(0, 2, 1)[..., None]
    lse = torch.logsumexp(s, dim=-1)
    o = torch.softmax(s, dim=-1) @ v
    return o.permute(0, 2, 1, 3).reshape(qkv.shape[0], qkv.shape[1], -1), lse


def closed_form_bwd(qkv, tau, query_bbox, num_heads, pc_range, out, lse, grad_out):
    """The backward rac_sasa_bwd implements, from the saved out and lse: -> (grad_qkv [B,Q,3E], grad_tau [B,Q,heads])"""
    B, Q, _ = query_bbox.shape
    q, k, v = _split(qkv, num_heads)
    d = q.shape[-1]
    r = _dist(query_bbox, pc_range)[:, None]
    s = (q / math.sqrt(d)) @ k.transpose(-1, -2) - r * tau.double().permute(0, 2, 1)[..., None]
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


def reference_with_scales(qkv, tau, query_bbox, num_heads, pc_range, grad_out, drop_key=None):
    """Float64 backward of the core (on the tensors' device) and, per kind, the magnitude A of the same computation with every
    term made non-negative: the bound of tests/test_sasa_grad_gpu.py is |got - ref| <= K * 2**-24 * A.
      S : A_S = |q/sqrt(d)|.|k| + (r + |c_i| + |c_j|) |tau| + |lse|   (a centre is formed in f32 from metres-sized values)
      P : A_P = P (A_S + max_j A_S)                                       (exp(s - lse): s and lse both rounded)
      dS: A_dS = A_P |dP - D| + P (|dO|.|v| + |dO|.|O|);  dq, dk, dv, dtau: products of these and the non-negative operands.
    ``drop_key``: key index removed from every row of (batch 0, head 0) in the returned gradients (a negative control); the
    A terms stay those of the full computation.  -> (dict kind -> (ref, A)) with kinds dq, dk, dv [B,Q,heads*d], dtau
    [B,Q,heads], lse [B,heads,Q]."""
    B, Q, _ = query_bbox.shape
    q, k, v = _split(qkv, num_heads)
    d = q.shape[-1]
    qs = q / math.sqrt(d)
    with torch.no_grad():
        c = R.decode_bbox(R.theta_d2xy(query_bbox.double()), pc_range)[..., :2]
    r = (c[:, :, None] - c[:, None]).norm(dim=-1)[:, None]                  # [B,1,Q,Q]
    cn = c.norm(dim=-1)
    csum = (cn[:, :, None] + cn[:, None])[:, None]
    ta = tau.double().permute(0, 2, 1)[..., None]                           # [B,H,Q,1]
    s = qs @ k.transpose(-1, -2) - r * ta
    lse_full = torch.logsumexp(s, dim=-1)
    if drop_key is not None:
        s = s.clone()
        s[0, 0, :, drop_key] = -math.inf
    lse = torch.logsumexp(s, dim=-1)
    P = torch.exp(s - lse[..., None])
    dO = grad_out.double().reshape(B, Q, num_heads, d).permute(0, 2, 1, 3)
    O = P @ v
    D = (dO * O).sum(-1, keepdim=True)
    dP = dO @ v.transpose(-1, -2)
    dS = P * (dP - D)
    AS = qs.abs() @ k.abs().transpose(-1, -2) + (r + csum) * ta.abs() + lse_full.abs()[..., None]
    AP = P * (AS + AS.amax(-1, keepdim=True))
    AdS = AP * (dP - D).abs() + P * (dO.abs() @ v.abs().transpose(-1, -2) + (dO.abs() * O.abs()).sum(-1, keepdim=True))
    T_ = AdS + dS.abs()

    def rows(x):
        return x.permute(0, 2, 1, 3).reshape(B, Q, -1)

    return {
        "dq": (rows(dS @ k / math.sqrt(d)), rows(T_ @ k.abs() / math.sqrt(d))),
        "dk": (rows(dS.transpose(-1, -2) @ qs), rows(T_.transpose(-1, -2) @ qs.abs())),
        "dv": (rows(P.transpose(-1, -2) @ dO), rows((AP + P).transpose(-1, -2) @ dO.abs())),
        "dtau": ((-(dS * r).sum(-1)).permute(0, 2, 1), ((T_ * r).sum(-1) + (dS.abs() * csum).sum(-1)).permute(0, 2, 1)),
        "lse": (lse, (P * AS).sum(-1) + AS.amax(-1)),
    }
