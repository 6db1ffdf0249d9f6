"""Float64 restatement of the AdaptiveMixing core and of the closed-form backward rac_mixing_bwd implements (test
infrastructure, shared by tests/test_mixing_grad_cpu.py and tests/test_mixing_grad_gpu.py).

Per (query, group) item, with LN over the whole [rows, 64] tile (no affine, biased variance, eps 1e-5):
    A = x M [P,64],  A^ = LN(A),  Y = relu(A^);   B = S Y [128,64],  B^ = LN(B),  Z = relu(B^)."""
import torch

EPS = 1e-5


def split_params(params, P, G):
    """params [B,Q,G*(64*64+128*P)] (any row stride) -> M [N,G,64,64], S [N,G,128,P] as float64, N = B*Q"""
    B, Q, _ = params.shape
    p = params.double().reshape(B * Q, G, 64 * 64 + 128 * P)
    return p[..., :4096].reshape(B * Q, G, 64, 64), p[..., 4096:].reshape(B * Q, G, 128, P)


def _ln(t):
    mu = t.mean(dim=(-2, -1), keepdim=True)
    var = ((t - mu) ** 2).mean(dim=(-2, -1), keepdim=True)
    r = 1.0 / torch.sqrt(var + EPS)
    return (t - mu) * r, r


def forward64(x, params, P, G):
    """-> dict of the float64 intermediates (x [N,G,P,64], M, S, A, Ah, r1, Y, B, Bh, r2, Z); differentiable in x and params"""
    Bn, Q = x.shape[:2]
    xx = x.double().reshape(Bn * Q, G, P, 64)
    M, S = split_params(params, P, G)
    A = xx @ M
    Ah, r1 = _ln(A)
    Y = torch.relu(Ah)
    Bm = S @ Y
    Bh, r2 = _ln(Bm)
    return dict(x=xx, M=M, S=S, A=A, Ah=Ah, r1=r1, Y=Y, B=Bm, Bh=Bh, r2=r2, Z=torch.relu(Bh))


def core64(x, params, P, G):
    """-> Z as [B,Q,G*128*64], float64"""
    Bn, Q = x.shape[:2]
    return forward64(x, params, P, G)["Z"].reshape(Bn, Q, -1)


def _ln_bwd(g, h, r):
    n = g.shape[-2] * g.shape[-1]
    mg = g.sum(dim=(-2, -1), keepdim=True) / n
    mgh = (g * h).sum(dim=(-2, -1), keepdim=True) / n
    return r * (g - mg - h * mgh), mg, mgh


def closed_form_bwd(x, params, grad_out, P, G):
    """The backward rac_mixing_bwd implements -> (grad_x [B,Q,G,P,64], grad_params [B,Q,G*(64*64+128*P)]), float64"""
    Bn, Q = x.shape[:2]
    with torch.no_grad():
        f = forward64(x, params, P, G)
        dZ = grad_out.double().reshape(Bn * Q, G, 128, 64)
        g2 = dZ * (f["Bh"] > 0)
        dB = _ln_bwd(g2, f["Bh"], f["r2"])[0]
        dS = dB @ f["Y"].transpose(-1, -2)
        dY = f["S"].transpose(-1, -2) @ dB
        g1 = dY * (f["Ah"] > 0)
        dA = _ln_bwd(g1, f["Ah"], f["r1"])[0]
        dM = f["x"].transpose(-1, -2) @ dA
        dx = dA @ f["M"].transpose(-1, -2)
    gp = torch.cat([dM.reshape(Bn * Q, G, -1), dS.reshape(Bn * Q, G, -1)], dim=-1).reshape(Bn, Q, -1)
    return dx.reshape(x.shape), gp


def min_margin(x, params, P, G):
    """-> [N,G] the least |pre-activation| (A^ and B^) of every item, float64"""
    with torch.no_grad():
        f = forward64(x, params, P, G)
    return torch.minimum(f["Ah"].abs().amin(dim=(-2, -1)), f["Bh"].abs().amin(dim=(-2, -1)))


def _mean(t):
    return t.mean(dim=(-2, -1), keepdim=True)


def _ln_scale(t, At, h, r, own=2.0):
    """relative error scale of r = 1/sqrt(var + eps) and the scale of h = (t - mean) r, given A_t for t.  ``own``: the roundings
    of r itself, in the unit A_t is counted in (0: A_t is an absolute perturbation of t and only its first-order image is
    wanted, as tests/mixing_fwd_ref.py pushes the operand truncations of the split-precision kernel through the chain)"""
    d = (t - _mean(t)).abs()
    At_c = At + _mean(At)
    r_rel = _mean(d * At_c) * r * r + own
    return r * At_c + h.abs() * r_rel, r_rel


def reference_with_scales(x, params, grad_out, P, G, zero_row=None):
    """Float64 backward of the core and, per kind, the magnitude A of the same computation with every term made non-negative
    and every rounded quantity carrying its own scale: the bound of tests/test_mixing_grad_gpu.py is
    |got - ref| <= K * 2**-24 * A.
      A_A = |x| |M|;  A_A^ = r1 (A_A + mean A_A) + |A^| e1, with e1 the relative scale of r1 (from the variance's terms);
      Y, B = S Y, B^ likewise; dB, dY = S^T dB, dA; dS, dM, dx: products of the non-negative operands and their scales.
    ``zero_row``: (item, group, out point) whose dZ row is set to zero in the returned gradients (a negative control); the A
    terms stay those of the full computation.  -> dict kind -> (ref, A) with kinds dx [N,G,P,64], dM [N,G,64,64],
    dS [N,G,128,P]."""
    Bn, Q = x.shape[:2]
    with torch.no_grad():
        f = forward64(x, params, P, G)
        dZ = grad_out.double().reshape(Bn * Q, G, 128, 64)
        ax, aM, aS = f["x"].abs(), f["M"].abs(), f["S"].abs()
        AA = ax @ aM
        AAh, e1 = _ln_scale(f["A"], AA, f["Ah"], f["r1"])
        m1 = f["Ah"] > 0
        AY = AAh * m1
        AB = aS @ (f["Y"] + AY)
        ABh, e2 = _ln_scale(f["B"], AB, f["Bh"], f["r2"])
        m2 = f["Bh"] > 0
        g2a = (dZ * m2).abs()
        aBh, aAh = f["Bh"].abs(), f["Ah"].abs()
        dB_full = _ln_bwd(dZ * m2, f["Bh"], f["r2"])[0]
        AdB = f["r2"] * (g2a + _mean(g2a) + ABh * _mean(g2a * aBh) + aBh * _mean(g2a * (aBh + ABh))) + dB_full.abs() * (e2 + 1.0)
        AdY = aS.transpose(-1, -2) @ (dB_full.abs() + AdB)
        dY_full = f["S"].transpose(-1, -2) @ dB_full
        g1a, Ag1 = (dY_full * m1).abs(), AdY * m1
        dA_full = _ln_bwd(dY_full * m1, f["Ah"], f["r1"])[0]
        AdA = f["r1"] * (Ag1 + _mean(Ag1 + g1a) + AAh * _mean(g1a * aAh) + aAh * _mean(Ag1 * aAh + g1a * (aAh + AAh))) \
            + dA_full.abs() * (e1 + 1.0)
        AdS = dB_full.abs() @ (f["Y"] + AY).transpose(-1, -2) + AdB @ f["Y"].transpose(-1, -2)
        AdM = ax.transpose(-1, -2) @ (dA_full.abs() + AdA)
        Adx = (dA_full.abs() + AdA) @ aM.transpose(-1, -2)

        if zero_row is not None:
            dZ = dZ.clone()
            dZ[zero_row[0], zero_row[1], zero_row[2]] = 0.0
        dB = _ln_bwd(dZ * m2, f["Bh"], f["r2"])[0]
        dS = dB @ f["Y"].transpose(-1, -2)
        dA = _ln_bwd((f["S"].transpose(-1, -2) @ dB) * m1, f["Ah"], f["r1"])[0]
        dM = f["x"].transpose(-1, -2) @ dA
        dx = dA @ f["M"].transpose(-1, -2)
    return {"dx": (dx, Adx), "dM": (dM, AdM), "dS": (dS, AdS)}
