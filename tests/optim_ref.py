"""Shared by the optimiser tests: the seeded case (tensor sizes at the kernels' edges, mixed learning rates and decays, gradient scales
that make some steps clip), and the references -- ``torch.optim.AdamW(foreach=False)`` after ``clip_grad_norm_`` on the CPU, in float64
(the truth) and in float32 (whose distance from the truth is the measure E_ref of the tests' allowance)."""
import torch

from racformer_amd.optim import CHUNK

SIZES = [1, 3, 5, 64, 255, 256, 257, 4096, 4097, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
MISALIGNED = SIZES.index(CHUNK + 1)     # this tensor's gradient is a view starting one element into a larger buffer
NO_GRAD, FROZEN = len(SIZES), len(SIZES) + 1        # indices of the parameter that never gets a gradient and of the frozen one
EXTRA_SIZES = [100, 50]
BASES = (1e-3, 1.0, 30.0)
STEPS = 3
CLIP = dict(max_norm=35, norm_type=2)
BETAS, EPS = (0.9, 0.999), 1e-8
_CACHE = {}


def hyper(i):
    """(lr, weight_decay) of tensor i: the recipe's two learning rates, with and without decay, in all four combinations"""
    return (4e-4 if i % 2 == 0 else 4e-5), (0.01 if (i // 2) % 2 == 0 else 0.0)


def make_case(seed, base):
    """float32 CPU tensors: ``params`` (the 13 sizes, then the one without a gradient and the frozen one) and ``grads[step][i]`` for
    the 13, tensor i scaled by ``base * 10^(-2 .. 2)``.  Shared; not modified."""
    key = ("case", seed, base)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(seed)
        params = [torch.randn(n, generator=g) for n in SIZES + EXTRA_SIZES]
        scales = [base * 10.0 ** (-2.0 + 4.0 * i / (len(SIZES) - 1)) for i in range(len(SIZES))]
        grads = [[torch.randn(n, generator=g) * s for n, s in zip(SIZES, scales)] for _ in range(STEPS)]
        _CACHE[key] = dict(params=params, grads=grads)
    return _CACHE[key]


def groups(params):
    out = []
    for i, p in enumerate(params):
        lr, wd = hyper(i)
        out.append(dict(params=[p], lr=lr, weight_decay=wd))
    return out


def leaves(case, dtype=torch.float32, device="cpu"):
    """Fresh parameters of the case (the frozen one with requires_grad off)."""
    ps = [torch.nn.Parameter(p.to(device=device, dtype=dtype).clone()) for p in case["params"]]
    ps[FROZEN].requires_grad_(False)
    return ps


def set_grads(ps, grads, misaligned=True):
    """``p.grad`` for the 13 (fresh tensors of the parameters' dtype and device; the MISALIGNED one a view one element into a larger
    buffer, which leaves it 4 bytes past a 16-byte boundary); the other two get none."""
    for i, g in enumerate(grads):
        p = ps[i]
        g = g.to(device=p.device, dtype=p.dtype)
        if misaligned and i == MISALIGNED:
            buf = torch.zeros(g.numel() + 8, dtype=p.dtype, device=p.device)
            buf[1:1 + g.numel()] = g
            g = buf[1:1 + g.numel()]
        else:
            g = g.clone()
        p.grad = g
    ps[NO_GRAD].grad = None
    ps[FROZEN].grad = None


def torch_reference(seed, base, dtype, clip=CLIP):
    """``clip_grad_norm_`` + ``torch.optim.AdamW(foreach=False)`` on the CPU in ``dtype`` -> per step a dict of lists ``p``, ``m``, ``v``
    (None where torch holds no state), plus ``norm`` (the norm torch clipped by).  Computed once per key; shared, not modified."""
    key = ("ref", seed, base, dtype, None if clip is None else clip["max_norm"])
    if key in _CACHE:
        return _CACHE[key]
    case = make_case(seed, base)
    ps = leaves(case, dtype)
    opt = torch.optim.AdamW(groups(ps), lr=1e-3, betas=BETAS, eps=EPS, foreach=False)
    out = []
    for s in range(STEPS):
        set_grads(ps, case["grads"][s], misaligned=False)
        norm = None
        if clip is not None:
            norm = torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], clip["max_norm"], clip["norm_type"], foreach=False)
        opt.step()
        out.append(snapshot(opt, ps, norm))
    _CACHE[key] = out
    return out


def snapshot(opt, ps, norm=None):
    st = [opt.state.get(p, {}) for p in ps]
    return dict(p=[p.detach().cpu().clone() for p in ps],
                m=[s["exp_avg"].detach().cpu().clone() if "exp_avg" in s else None for s in st],
                v=[s["exp_avg_sq"].detach().cpu().clone() if "exp_avg_sq" in s else None for s in st],
                step=[float(s["step"]) if "step" in s else None for s in st], norm=None if norm is None else float(norm))


def bits(t):
    return t.detach().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int64).cpu()
