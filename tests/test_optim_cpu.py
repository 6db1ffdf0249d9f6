"""racformer_amd.optim without a GPU: FusedAdamW's torch route against torch.optim.AdamW + clip_grad_norm_ in float64, the optimiser
constructor's precedence rule, the scheduler's closed forms, parse_losses, and state dicts exchanged with torch.optim.AdamW."""
import ctypes
import math

import pytest
import torch
import torch.nn as nn

import optim_ref as OR
from racformer_amd import _lib
from racformer_amd import optim as O


@pytest.mark.parametrize("clip", [OR.CLIP, None], ids=["clipped", "unclipped"])
@pytest.mark.parametrize("base", OR.BASES)
def test_torch_route_in_float64(base, clip):
    """3 steps in float64 against torch.optim.AdamW(foreach=False) + clip_grad_norm_: relative difference at most 1e-14"""
    case = OR.make_case(3, base)
    want = OR.torch_reference(3, base, torch.float64, clip)
    ps = OR.leaves(case, torch.float64)
    opt = O.FusedAdamW(OR.groups(ps), betas=OR.BETAS, eps=OR.EPS, grad_clip=clip)
    versions = [p._version for p in ps]
    for s in range(OR.STEPS):
        OR.set_grads(ps, case["grads"][s])
        before = [g.clone() for g in (p.grad for p in ps[:len(OR.SIZES)])]
        opt.step()
        assert all(torch.equal(p.grad, b) for p, b in zip(ps, before)), "the gradients are left unclipped"
        got = OR.snapshot(opt, ps)
        if clip is not None:
            assert abs(float(opt.grad_norm) - want[s]["norm"]) <= 1e-14 * want[s]["norm"]
            clipped = want[s]["norm"] > clip["max_norm"]
            assert (float(opt.clip_coef) < 1.0) == clipped
        else:
            assert float(opt.clip_coef) == 1.0
        assert int(opt.skipped) == 0
        worst = 0.0
        for k in ("p", "m", "v"):
            for i, (a, b) in enumerate(zip(got[k], want[s][k])):
                assert (a is None) == (b is None), f"{k}[{i}]: state held on one side only"
                if a is not None:
                    worst = max(worst, float((a - b).abs().max() / b.abs().max()))
        assert got["step"] == want[s]["step"]
        print(f"base {base} step {s}: largest relative difference {worst:.3g}")
        assert worst <= 1e-14
    # both regimes occur over the bases (so the clip is exercised, and so is its absence)
    if clip is not None:
        assert (want[0]["norm"] > clip["max_norm"]) == (base >= 1.0)
    assert torch.equal(ps[OR.NO_GRAD], case["params"][OR.NO_GRAD].double()) and torch.equal(ps[OR.FROZEN], case["params"][OR.FROZEN].double())
    assert ps[OR.NO_GRAD] not in opt.state and ps[OR.FROZEN] not in opt.state
    assert [p._version > v for p, v in zip(ps, versions)] == [True] * len(OR.SIZES) + [False, False]


def test_torch_route_skips_a_non_finite_step():
    case = OR.make_case(3, 1.0)
    ps = OR.leaves(case)
    opt = O.FusedAdamW(OR.groups(ps), grad_clip=OR.CLIP)
    OR.set_grads(ps, case["grads"][0])
    opt.step()
    before = OR.snapshot(opt, ps)
    for bad in (float("inf"), float("nan")):
        OR.set_grads(ps, case["grads"][1])
        ps[7].grad[11] = bad
        opt.step()
        after = OR.snapshot(opt, ps)
        assert int(opt.skipped) == 1 and after["step"] == before["step"]
        for k in ("p", "m", "v"):
            assert all(a is b or torch.equal(OR.bits(a), OR.bits(b)) for a, b in zip(after[k], before[k]))


def test_refusals_and_moment_layout():
    with pytest.raises(NotImplementedError):
        O.FusedAdamW([nn.Parameter(torch.zeros(3))], grad_clip=dict(max_norm=1.0, norm_type=1))
    with pytest.raises(NotImplementedError):
        O.FusedAdamW([nn.Parameter(torch.zeros(3))], amsgrad=True)
    with pytest.raises(ValueError):
        O.FusedAdamW([nn.Parameter(torch.zeros(3, dtype=torch.float16))])
    ps = [nn.Parameter(torch.ones(n)) for n in (3, 5, 64, 1)]
    opt = O.FusedAdamW(ps, lr=1e-3)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step()
    m0 = opt.state[ps[0]]["exp_avg"]
    for p in ps:
        s = opt.state[p]
        assert s["exp_avg"].shape == p.shape and s["exp_avg_sq"].shape == p.shape and s["step"].dtype == torch.float32
        for k in ("exp_avg", "exp_avg_sq"):
            assert (s[k].data_ptr() - opt.state[ps[0]][k].data_ptr()) % 16 == 0, "per-tensor views start at 16-byte-aligned offsets"
            assert s[k].untyped_storage().data_ptr() == opt.state[ps[0]][k].untyped_storage().data_ptr(), "one flat buffer"
    assert m0.data_ptr() % 16 == 0
    # the C entry checks its arguments before any HIP call
    lib = _lib.lib()
    assert lib.rac_adamw_step(None, 1, None, 1, None, None, None, None, None, 1.0, _lib.OPT_ALL, None) == -1
    assert b"null pointer" in lib.rac_last_error()
    one = ctypes.c_void_p(64)
    assert lib.rac_adamw_step(one, 2, one, 1, one, one, one, one, one, 1.0, _lib.OPT_ALL, None) == -1 and b"n_chunks" in lib.rac_last_error()
    assert lib.rac_adamw_step(one, 1, one, 1, one, one, one, one, one, 1.0, 8, None) == -1 and b"phases" in lib.rac_last_error()
    assert lib.rac_adamw_step(one, 1, one, 1, one, one, one, one, one, float("nan"), 7, None) == -1 and b"max_norm" in lib.rac_last_error()


def test_header_constants_match_the_binding():
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "racformer_hip.h")).read()
    want = {k: int(v) for k, v in re.findall(r"#define\s+RAC_OPT_(CHUNK|HYPER|SCALARS)\s+(\d+)", text)}
    assert want == dict(CHUNK=_lib.OPT_CHUNK, HYPER=_lib.OPT_HYPER, SCALARS=_lib.OPT_SCALARS) and O.CHUNK == _lib.OPT_CHUNK
    assert re.search(r"RAC_OPT_NORM = 1, RAC_OPT_FINISH = 2, RAC_OPT_UPDATE = 4, RAC_OPT_ALL = 7", text)
    assert (_lib.OPT_NORM, _lib.OPT_FINISH, _lib.OPT_UPDATE, _lib.OPT_ALL) == (1, 2, 4, 7)
    # rac_opt_tensor: four pointers, int64, two int32; rac_opt_chunk: int64, two int32
    assert O._TENSOR.itemsize == 48 and O._CHUNK.itemsize == 16
    assert [O._TENSOR.fields[n][1] for n in ("p", "g", "m", "v", "numel", "row")] == [0, 8, 16, 24, 32, 40]
    assert [O._CHUNK.fields[n][1] for n in ("start", "tensor")] == [0, 8]


class Toy(nn.Module):
    def __init__(self):
        super().__init__()
        self.img_backbone = nn.Module()
        self.img_backbone.layer1 = nn.Module()
        self.img_backbone.layer1.w = nn.Parameter(torch.zeros(4))
        self.img_backbone.sampling_offset = nn.Module()             # matches both keys: the longer one wins
        self.img_backbone.sampling_offset.w = nn.Parameter(torch.zeros(4))
        self.img_backbone.stem = nn.Parameter(torch.zeros(4), requires_grad=False)
        self.x = nn.Module()
        self.x.sampling_offset = nn.Linear(2, 2)
        self.head = nn.Module()
        self.head.w = nn.Parameter(torch.zeros(4))


def test_build_optimizer_precedence():
    toy = Toy()
    cfg = dict(type='AdamW', lr=4e-4, weight_decay=0.01, grad_clip=dict(max_norm=35, norm_type=2),
               paramwise_cfg=dict(custom_keys={'img_backbone': dict(lr_mult=0.1), 'sampling_offset': dict(lr_mult=0.5, decay_mult=0.0)}))
    opt = O.build_optimizer(toy, cfg)
    names = [n for n, _ in toy.named_parameters()]
    assert len(opt.param_groups) == len(names) and all(len(g["params"]) == 1 for g in opt.param_groups)
    got = {n: (g["lr"], g["weight_decay"]) for n, g in zip(names, opt.param_groups)}
    assert got["img_backbone.layer1.w"] == (4e-4 * 0.1, 0.01 * 1.0)
    assert got["x.sampling_offset.bias"] == (4e-4 * 0.5, 0.0) and got["x.sampling_offset.weight"] == (4e-4 * 0.5, 0.0)
    assert got["head.w"] == (4e-4, 0.01)
    assert got["img_backbone.stem"] == (4e-4, 0.01), "a frozen parameter passes through with the defaults"
    # both keys are substrings; sorted alphabetically, then by length with the longest first: 'sampling_offset' (15) before 'img_backbone' (12)
    assert got["img_backbone.sampling_offset.w"] == (4e-4 * 0.5, 0.0)
    assert opt.max_norm == 35.0
    # keys of equal length: the alphabetical order decides (stable sort), so 'aa' is tried before 'bb'
    class Two(nn.Module):
        def __init__(self):
            super().__init__()
            self.aa_bb = nn.Parameter(torch.zeros(1))
    o2 = O.build_optimizer(Two(), dict(type='AdamW', lr=1.0, paramwise_cfg=dict(custom_keys={'bb': dict(lr_mult=3.0), 'aa': dict(lr_mult=2.0)})))
    assert o2.param_groups[0]["lr"] == 2.0
    with pytest.raises(NotImplementedError):
        O.build_optimizer(toy, dict(type='SGD', lr=0.1))
    single = O.build_optimizer(toy, dict(type='AdamW', lr=4e-4, weight_decay=0.01))
    assert len(single.param_groups) == 1 and len(single.param_groups[0]["params"]) == len(names)


def test_scheduler_closed_forms():
    toy = Toy()
    opt = O.build_optimizer(toy, dict(type='AdamW', lr=4e-4, weight_decay=0.01,
                                      paramwise_cfg=dict(custom_keys={'img_backbone': dict(lr_mult=0.1), 'sampling_offset': dict(lr_mult=0.1)})))
    names = [n for n, _ in toy.named_parameters()]
    sched = O.CosineAnnealingLr(opt, max_epochs=36, warmup='linear', warmup_iters=500, warmup_ratio=1.0 / 3, min_lr_ratio=1e-3)

    def lrs():
        return {n: g["lr"] for n, g in zip(names, opt.param_groups)}

    def check(want):
        got = lrs()
        assert math.isclose(got["head.w"], want, rel_tol=1e-12, abs_tol=0.0), (got["head.w"], want)
        for n in names:
            mult = 1.0 if n in ("head.w", "img_backbone.stem") else 0.1        # (the frozen stem passed through without a multiplier)
            assert math.isclose(got[n], mult * want, rel_tol=1e-12, abs_tol=0.0), (n, got[n], mult * want)
            # the lr_mult groups sit at 0.1x: the schedule is linear in the base, so only roundings (a few 2^-53) separate them
            assert math.isclose(got[n], mult * got["head.w"], rel_tol=2e-15, abs_tol=0.0), (n, got[n], got["head.w"])

    sched.before_train_epoch(0)
    check(4e-4)
    sched.before_train_iter(0)
    check(4e-4 / 3)
    sched.before_train_iter(250)
    check(4e-4 * 2 / 3)
    sched.before_train_iter(500)
    check(4e-4)
    sched.before_train_iter(501)
    check(4e-4)
    sched.before_train_epoch(18)
    sched.before_train_iter(18 * 1000)
    check(2.002e-4)
    sched.before_train_epoch(36)
    check(4e-4 * 1e-3)
    # warm-up scales the epoch's regular value, not the base: iteration 250 of an epoch-1 schedule
    sched.before_train_epoch(1)
    regular = 4e-7 + 0.5 * (4e-4 - 4e-7) * (math.cos(math.pi / 36) + 1)
    sched.before_train_iter(250)
    check(regular * 2 / 3)


def test_parse_losses():
    losses = dict(loss_cls=torch.tensor([1.0, 3.0]), loss_bbox=[torch.tensor([2.0, 4.0]), torch.tensor(1.0)], acc=torch.tensor(90.0),
                  **{"d0.loss_cls_dn": torch.tensor(0.5)})
    total, log_vars = O.parse_losses(losses)
    assert float(total) == 2.0 + 4.0 + 0.5                   # the means; the non-loss key stays out of the total
    assert list(log_vars) == ["loss_cls", "loss_bbox", "acc", "d0.loss_cls_dn", "loss"]
    assert float(log_vars["acc"]) == 90.0 and float(log_vars["loss"]) == 6.5 and float(log_vars["loss_bbox"]) == 4.0
    assert all(isinstance(v, torch.Tensor) and not v.requires_grad for v in log_vars.values())
    w = torch.ones(2, requires_grad=True)
    total, log_vars = O.parse_losses(dict(loss_a=(w * 2).sum()))
    total.backward()
    assert torch.equal(w.grad, torch.full((2,), 2.0)) and not log_vars["loss"].requires_grad
    with pytest.raises(TypeError):
        O.parse_losses(dict(loss=1.0))


def test_train_step_order():
    """zero_grad, the model's losses, backward, step: one call moves the weights by exactly one clipped AdamW step"""
    class M(nn.Module):
        def __init__(self):
            super().__init__()
            self.w = nn.Parameter(torch.tensor([1.0, -2.0, 3.0]))

        def forward(self, return_loss=True, x=None):
            assert return_loss
            return dict(loss_a=(self.w * x).sum(), loss_b=[(self.w ** 2).sum()], other=self.w.detach().sum())

    a, b = M(), M()
    a.w.grad = torch.full((3,), 1e9)                       # stale: train_step drops it before the backward
    opt = O.FusedAdamW(a.parameters(), lr=1e-2, weight_decay=0.1, grad_clip=dict(max_norm=0.5))
    x = torch.tensor([0.5, 0.25, -1.0])
    log_vars = O.train_step(a, opt, x=x)
    ref = torch.optim.AdamW(b.parameters(), lr=1e-2, weight_decay=0.1, foreach=False)
    ((b.w * x).sum() + (b.w ** 2).sum()).backward()
    torch.nn.utils.clip_grad_norm_(b.parameters(), 0.5)
    ref.step()
    assert torch.allclose(a.w, b.w, rtol=1e-6, atol=0) and set(log_vars) == {"loss_a", "loss_b", "other", "loss"}


@pytest.mark.parametrize("direction", ["torch_to_fused", "fused_to_torch"])
def test_state_dict_round_trip(direction):
    """two steps with one optimiser, its state dict into the other, a third step with both: the same parameters as three steps of one"""
    case = OR.make_case(5, 1e-3)

    def make(kind, ps):
        if kind == "torch":
            return torch.optim.AdamW(OR.groups(ps), lr=1e-3, betas=OR.BETAS, eps=OR.EPS, foreach=False)
        return O.FusedAdamW(OR.groups(ps), lr=1e-3, betas=OR.BETAS, eps=OR.EPS)

    first, second = direction.split("_to_")
    ps = OR.leaves(case, torch.float64)
    opt = make(first, ps)
    for s in range(2):
        OR.set_grads(ps, case["grads"][s])
        opt.step()
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and sorted(sd["state"]) == list(range(len(OR.SIZES)))
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} and float(s["step"]) == 2.0 for s in sd["state"].values())
    if first == "fused":        # what was saved does not alias the optimiser's flat buffers
        assert all(sd["state"][0][k].data_ptr() != opt.state[ps[0]][k].data_ptr() for k in ("step", "exp_avg", "exp_avg_sq"))
    ps2 = [nn.Parameter(p.detach().clone(), requires_grad=p.requires_grad) for p in ps]
    opt2 = make(second, ps2)
    opt2.load_state_dict(sd)
    for o, q in ((opt, ps), (opt2, ps2)):
        OR.set_grads(q, case["grads"][2])
        o.step()
    want = OR.torch_reference(5, 1e-3, torch.float64, None)[2]
    for q, o in ((ps, opt), (ps2, opt2)):
        got = OR.snapshot(o, q)
        for k in ("p", "m", "v"):
            for a, b in zip(got[k], want[k]):
                assert (a is None) == (b is None)
                assert a is None or float((a - b).abs().max() / b.abs().max()) <= 1e-14
        assert got["step"] == want["step"]
