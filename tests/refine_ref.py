"""torch restatement of the box-refinement tail of a decoder layer and of its closed-form backward (what rac_refine_fwd /
rac_refine_bwd compute), written from the reference: refine_bbox (models/racformer_transformer.py:230-236), the velocity
scaling (:265-269), inverse_sigmoid (models/utils.py:86-101) and theta_d2xy_coods (models/bbox/utils.py:82-90).

  forward          the reference's ops in the dtype of its inputs -> (bbox_pred, bbox_xy); differentiable by autograd
  closed_form_bwd  float64 (grad_pred, grad_xy) -> (grad_delta, grad_proposal), with torch's gates: clamp passes the gradient on
                   the closed interval; ``magnitude=True``: the same sums with every term made non-negative -- the scale A of the
                   error metric worst |err| / A in units of 2^-24
  gate_margins     how far every row keeps from a gate it is not exactly on
  make_case        seeded inputs with rows placed on the gates
"""
import math

import torch

EPS = 1e-5
MAP, RADIUS = 102.4, 65.0
UNIT = 2.0 ** -24


def inverse_sigmoid(x, eps=EPS):
    x = x.clamp(min=0, max=1)
    x1 = x.clamp(min=eps)
    x2 = (1 - x).clamp(min=eps)
    return torch.log(x1 / x2)


def forward(proposal, delta, time_diff_safe, num_ray):
    """proposal, delta [B,Q,10], time_diff_safe [B,T] (time_diff with values < 1e-5 replaced by 1) -> (bbox_pred, bbox_xy)"""
    dz_new = torch.sigmoid(delta[..., 1:3] + inverse_sigmoid(proposal[..., 1:3]))
    theta = proposal[..., 0:1] + (torch.sigmoid(delta[..., 0:1]) * 2 - 1) / num_ray
    vel = delta[..., 8:]
    if time_diff_safe.shape[1] > 1:
        vel = vel / time_diff_safe[:, 1:2, None]
    pred = torch.cat([theta, dz_new, delta[..., 3:8], vel], dim=-1)
    center = MAP / 2
    ang, rad = pred[..., 0:1] * (2 * math.pi), pred[..., 1:2] * RADIUS
    xy = torch.cat([(center + rad * torch.cos(ang)) / MAP, (center + rad * torch.sin(ang)) / MAP], dim=-1)
    return pred, torch.cat([torch.clamp(xy, min=0, max=1), pred[..., 2:]], dim=-1)


def _pre_clamp_xy(proposal, delta, num_ray):
    p, d = proposal.double(), delta.double()
    o0 = p[..., 0] + (torch.sigmoid(d[..., 0]) * 2 - 1) / num_ray
    o1 = torch.sigmoid(d[..., 1] + inverse_sigmoid(p[..., 1]))
    ang, rad = o0 * (2 * math.pi), o1 * RADIUS
    return (MAP / 2 + rad * torch.cos(ang)) / MAP, (MAP / 2 + rad * torch.sin(ang)) / MAP, ang, rad


def closed_form_bwd(proposal, delta, time_diff_safe, num_ray, grad_pred=None, grad_xy=None, magnitude=False):
    """float64 closed form; an absent gradient counts as zero"""
    p, d, td = proposal.double(), delta.double(), time_diff_safe.double()
    ab = (lambda x: x.abs()) if magnitude else (lambda x: x)
    sub = (lambda x, y: x + y) if magnitude else (lambda x, y: x - y)
    go = [ab(grad_pred.double()[..., k]) if grad_pred is not None else torch.zeros_like(p[..., 0]) for k in range(10)]
    ux, uy, ang, rad = _pre_clamp_xy(proposal, delta, num_ray)
    s0 = torch.sigmoid(d[..., 0])
    o = [None, torch.sigmoid(d[..., 1] + inverse_sigmoid(p[..., 1])), torch.sigmoid(d[..., 2] + inverse_sigmoid(p[..., 2]))]
    if grad_xy is not None:
        gx = grad_xy.double()
        gux = torch.where((ux >= 0) & (ux <= 1), ab(gx[..., 0]) / MAP, torch.zeros_like(ux))
        guy = torch.where((uy >= 0) & (uy <= 1), ab(gx[..., 1]) / MAP, torch.zeros_like(uy))
        cs, sn = ab(torch.cos(ang)), ab(torch.sin(ang))
        go[0] = go[0] + sub(guy * cs, gux * sn) * rad * (2 * math.pi)
        go[1] = go[1] + (gux * cs + guy * sn) * RADIUS
        for k in range(2, 10):
            go[k] = go[k] + ab(gx[..., k])
    gd, gp = [None] * 10, [torch.zeros_like(p[..., 0]) for _ in range(10)]
    gd[0] = go[0] * (2 * s0 * (1 - s0) / num_ray)
    gp[0] = go[0]
    for k in (1, 2):
        x = p[..., k]
        gs = go[k] * o[k] * (1 - o[k])
        inside = (x >= 0) & (x <= 1)
        zero = torch.zeros_like(x)
        jac = torch.where(inside & (x >= EPS), 1 / x.clamp(min=EPS), zero) + \
            torch.where(inside & (1 - x >= EPS), 1 / (1 - x).clamp(min=EPS), zero)
        gd[k], gp[k] = gs, gs * jac
    for k in range(3, 10):
        gd[k] = go[k]
    if td.shape[1] > 1:
        for k in (8, 9):
            gd[k] = gd[k] / td[:, 1:2]
    return torch.stack(gd, dim=-1), torch.stack(gp, dim=-1)


INPUT_MARGIN, COMPUTED_MARGIN = 1e-6, 1e-5


def gate_margins(proposal, delta, num_ray):
    """(input, computed): the smallest distance of a row to a gate it is not exactly on.  Input gates compare proposal[1:3] itself
    -- a value float32 and float64 read identically -- with 0, 1, eps and 1 - eps; only the rounding of the constant eps can make
    the two precisions disagree there (the window (0, eps) is itself 1e-5 wide, so it cannot hold a margin of 1e-5: 1e-6 is asked).
    Computed gates compare the pre-clamp xy, which each precision rounds its own way, with 0 and 1: 1e-5 is asked, and no row can
    be placed exactly on them."""
    x = proposal.double()[..., 1:3].reshape(-1)
    dist = torch.stack([x.abs(), (x - 1).abs(), (x - EPS).abs(), (1 - x - EPS).abs()])
    exact = torch.stack([x == 0, x == 1, torch.zeros_like(x, dtype=torch.bool), torch.zeros_like(x, dtype=torch.bool)])
    inp = float(torch.where(exact, torch.full_like(dist, float("inf")), dist).min())
    ux, uy, _, _ = _pre_clamp_xy(proposal, delta, num_ray)
    u = torch.cat([ux.reshape(-1), uy.reshape(-1)])
    return inp, float(torch.minimum(u.abs(), (u - 1).abs()).min())


def make_case(seed, B, Q, T, one_at=None):
    """float32 (proposal, delta, time_diff_safe, grad_pred, grad_xy).  The first rows of every batch sit on the gates: proposal[1]
    / proposal[2] exactly 0 and exactly 1, inside (0, eps) and inside (1 - eps, 1), below 0 and above 1; boxes whose xy leaves
    [0,1] on each of the four sides.  ``one_at``: batch whose time_diff_safe[:, 1] is 1.0 (a replaced time difference)."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)                         # noqa: E731
    prop = torch.cat([r(B, Q, 1), 0.05 + 0.9 * r(B, Q, 2), r(B, Q, 7) * 2 - 1], dim=-1)
    delta = torch.randn(B, Q, 10, generator=g) * 0.7
    special = [(0.0, 0.4), (1.0, 0.6), (0.3, 0.0), (0.7, 1.0), (4e-6, 0.5), (0.5, 1.0 - 4e-6), (-0.25, 0.5), (0.5, 1.25), (0.0, 1.0)]
    for i, (a, b) in enumerate(special):
        prop[:, i, 1], prop[:, i, 2] = a, b
    n = len(special)
    # (18 degrees off the axes: on an axis the blocked coordinate's sin / cos is the only term left and vanishes, and the metric
    #  would measure the rounding of the angle against a magnitude of zero)
    for i, turn in enumerate((0.05, 0.30, 0.55, 0.80)):                # x > 1, y > 1, x < 0, y < 0
        prop[:, n + i, 0], prop[:, n + i, 1], delta[:, n + i, 0], delta[:, n + i, 1] = turn, 0.97, 0.0, 1.5
    td = 0.3 + r(B, T)
    td[:, 0] = 1.0
    if one_at is not None and T > 1:
        td[one_at, 1] = 1.0
    gp = torch.randn(B, Q, 10, generator=g)
    gx = torch.randn(B, Q, 10, generator=g)
    return prop.float(), delta.float(), td.float(), gp.float(), gx.float()


def err_over_a(got, want, mag):
    """worst |got - want| / A in units of 2^-24, A = the magnitude sum (a floor keeps empty sums out)"""
    a = mag.clamp(min=1e-30)
    return float(((got.double().cpu() - want.cpu()).abs() / a.cpu()).max() / UNIT)
