"""FusedAdamW on the MI355X (rac_adamw_step, csrc/optimizer.hip): the update rule against float64, the norm's bits, skipped and
zero-gradient steps bit for bit, parameter versions, weight caches after a step (the detector offline and streaming, a bare neck), a
captured step against eager steps, and the refusals.

The update rule's allowance is the project's: max|kernel - float64| <= RATIO x E_ref + 2^-23 x scale per tensor and per quantity, E_ref
the error of torch's own CPU float32 AdamW(foreach=False) + clip_grad_norm_ against float64 on the same case, scale the largest |float64|
value of the tensor.  The norm's bound is derived: the squares of float32 values are exact in float64 and each side makes N - 1 float64
additions, so the two sums of squares differ by at most 2 N 2^-53 relative."""
import copy

import pytest
import torch
import torch.nn as nn

import detector_ref as DR
import detector_train_ref as TR
import necks_ref as NR
import optim_ref as OR
from racformer_amd import _lib, necks, optim as O
from racformer_amd import synthetic as syn
from test_depth_net_gpu import RATIO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 3
N_GRAD = sum(OR.SIZES)


def fused(case, clip=OR.CLIP):
    ps = OR.leaves(case, device=DEV)
    return ps, O.FusedAdamW(OR.groups(ps), betas=OR.BETAS, eps=OR.EPS, grad_clip=clip)


@pytest.mark.parametrize("base", OR.BASES)
def test_update_rule_three_steps(base):
    case = OR.make_case(SEED, base)
    want = OR.torch_reference(SEED, base, torch.float64)
    ref32 = OR.torch_reference(SEED, base, torch.float32)
    ps, opt = fused(case)
    clipped = []
    for s in range(OR.STEPS):
        OR.set_grads(ps, case["grads"][s])
        grads = [p.grad.clone() for p in ps[:len(OR.SIZES)]]
        opt.step()
        assert all(torch.equal(p.grad, g) for p, g in zip(ps, grads)), "the gradients are read, not written"
        clipped.append(float(opt.clip_coef) < 1.0)
        assert clipped[-1] == (want[s]["norm"] > OR.CLIP["max_norm"]) and int(opt.skipped) == 0
        # (torch's float64 norm is itself 7e-15 off the exactly rounded root on this case; test_norm holds the kernel to its own bound)
        assert abs(float(opt.grad_norm) - want[s]["norm"]) <= 1e-13 * want[s]["norm"]
    assert clipped == [base >= 1.0] * OR.STEPS                # over the bases some steps clip and some do not
    got = OR.snapshot(opt, ps)
    last = OR.STEPS - 1
    assert got["step"] == want[last]["step"] == [float(OR.STEPS)] * len(OR.SIZES) + [None, None]
    worst = 0.0
    for k in ("p", "m", "v"):
        for i, n in enumerate(OR.SIZES):
            w64 = want[last][k][i]
            e_ref = float((ref32[last][k][i].double() - w64).abs().max())
            err = float((got[k][i].double() - w64).abs().max())
            tol = RATIO * e_ref + 2.0 ** -23 * float(w64.abs().max())
            worst = max(worst, err / tol)
            assert err <= tol, f"{k} of tensor {i} ({n} elements): error {err:.3g}, allowed {tol:.3g} (E_ref {e_ref:.3g})"
    print(f"base {base}: the largest share of the allowance used is {worst:.3f}")
    for i in (OR.NO_GRAD, OR.FROZEN):
        assert torch.equal(OR.bits(ps[i]), OR.bits(case["params"][i])) and ps[i] not in opt.state


def norm_bits(case, step, shift=None):
    """The record of one step's norm; ``shift``: every gradient a view ``shift`` elements into one flat buffer (other addresses, and for
    shift % 4 != 0 the scalar loads), the parameters allocated after it."""
    if shift is not None:
        pad = torch.empty(12345 + shift, device=DEV)          # noqa: F841  (moves every later allocation)
    ps, opt = fused(case)
    OR.set_grads(ps, case["grads"][step])
    if shift is not None:
        flat = torch.zeros(N_GRAD + 4 * len(OR.SIZES) + 8, device=DEV)
        at = shift
        for p in ps[:len(OR.SIZES)]:
            view = flat[at:at + p.numel()]
            view.copy_(p.grad)
            p.grad = view
            at += p.numel()
    opt.step()
    return OR.bits(opt.grad_norm_sq), OR.bits(opt.grad_norm), float(opt.grad_norm_sq), float(opt.grad_norm)


@pytest.mark.parametrize("base", OR.BASES)
def test_norm(base):
    case = OR.make_case(SEED, base)
    sq64 = float(sum((g.double() * g.double()).sum() for g in case["grads"][0]))
    a = norm_bits(case, 0)
    rel = abs(a[2] - sq64) / sq64
    print(f"base {base}: sum of squares {a[2]!r} against {sq64!r}: relative {rel:.3g}, allowed {2 * N_GRAD * 2.0 ** -53:.3g}")
    assert rel <= 2 * N_GRAD * 2.0 ** -53
    assert abs(a[3] ** 2 - sq64) / sq64 <= 2 * N_GRAD * 2.0 ** -53, "opt.grad_norm squared"
    b = norm_bits(case, 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "two runs give other bits"
    for shift in (4, 1, 2, 3):
        c = norm_bits(case, 0, shift)
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]), f"other addresses (shift {shift}) give other bits"


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_non_finite_gradient_skips_the_step_bitwise(bad):
    case = OR.make_case(SEED, 1.0)
    ps, opt = fused(case)
    OR.set_grads(ps, case["grads"][0])
    opt.step()
    before = OR.snapshot(opt, ps)
    OR.set_grads(ps, case["grads"][1])
    ps[len(OR.SIZES) - 1].grad[2 * O.CHUNK + 77] = bad      # one element of one gradient
    opt.step()
    after = OR.snapshot(opt, ps)
    assert int(opt.skipped) == 1 and not bool(torch.isfinite(opt.grad_norm))
    assert after["step"] == before["step"] == [1.0] * len(OR.SIZES) + [None, None]
    for k in ("p", "m", "v"):
        for i, (x, y) in enumerate(zip(after[k], before[k])):
            assert (x is None and y is None) or torch.equal(OR.bits(x), OR.bits(y)), f"{k} of tensor {i} changed in a skipped step"
    OR.set_grads(ps, case["grads"][1])                      # the next finite step goes through
    opt.step()
    assert int(opt.skipped) == 0 and OR.snapshot(opt, ps)["step"][0] == 2.0


def test_zero_gradients_are_pure_decay():
    case = OR.make_case(SEED, 1.0)
    ps, opt = fused(case)
    OR.set_grads(ps, [torch.zeros_like(g) for g in case["grads"][0]])
    opt.step()
    assert float(opt.grad_norm) == 0.0 and float(opt.clip_coef) == 1.0 and int(opt.skipped) == 0
    for i in range(len(OR.SIZES)):
        lr, wd = OR.hyper(i)
        decay = torch.tensor(1.0 - lr * wd, dtype=torch.float64).float()
        assert torch.equal(OR.bits(ps[i]), OR.bits(case["params"][i] * decay)), f"tensor {i}"
        s = opt.state[ps[i]]
        assert not bool(s["exp_avg"].any()) and not bool(s["exp_avg_sq"].any()) and float(s["step"]) == 1.0


def test_versions_move_on_the_updated_parameters_only():
    case = OR.make_case(SEED, 1.0)
    ps, opt = fused(case)
    OR.set_grads(ps, case["grads"][0])
    before = [p._version for p in ps]
    opt.step()
    moved = [p._version > v for p, v in zip(ps, before)]
    assert moved == [True] * len(OR.SIZES) + [False, False]
    for i in (OR.NO_GRAD, OR.FROZEN):
        assert torch.equal(OR.bits(ps[i]), OR.bits(case["params"][i]))


def test_detector_serves_no_stale_packs_after_a_train_step():
    cfg = syn.SMALL
    det = DR.build(cfg).to(DEV)
    det.fused_grad = True
    opt = O.build_optimizer(det, dict(type='AdamW', lr=4e-4, weight_decay=0.01, grad_clip=dict(max_norm=35, norm_type=2),
                                      paramwise_cfg=dict(custom_keys={'img_backbone': dict(lr_mult=0.1), 'sampling_offset': dict(lr_mult=0.1)})))

    def infer(d):
        d.eval()
        out = [d.simple_test_offline(**DR.offline_args(cfg, [2, 1, 0], device=DEV))[0]["pts_bbox"]]
        for s, fids in enumerate(DR.sequence(2, cfg.num_frames)):     # (the second call replays a captured plan)
            img, points, depth, rcs, metas = DR.window_inputs(cfg, fids, sample=s, device=DEV)
            out.append(d.simple_test_online(metas, img, False, points, depth, rcs)[0]["pts_bbox"])
        d.reset_memory()
        return out

    try:
        old = infer(det)                                    # every weight-derived cache is warm, on the weights before the step
        det.train()
        state = copy.deepcopy(det.state_dict())
        TR.seed_all(7)
        log_vars = O.train_step(det, opt, **TR.train_args(cfg, (3,), device=DEV))
        assert bool(torch.isfinite(log_vars["loss"])) and log_vars["loss"].is_cuda and int(opt.skipped) == 0
        changed = [n for n, p in det.named_parameters() if not torch.equal(p, state[n])]
        assert len(changed) > 100
        got = infer(det)
        fresh = DR.build(cfg).to(DEV)
        fresh.fused_grad = True
        fresh.load_state_dict(det.state_dict())
        want = infer(fresh)
        for i, (g, w) in enumerate(zip(got, want)):
            assert DR.same_result(g, w), f"inference {i} after the step differs from a fresh detector on the updated weights"
        assert not all(DR.same_result(g, o) for g, o in zip(got, old)), "the step did not change the detections: the check shows nothing"
    finally:
        det.reset_memory()


def test_bare_neck_serves_no_stale_packs_after_a_step():
    def make():
        m = necks.CustomFPN(NR.LSS["channels"], 256, num_outs=1, start_level=0, out_ids=[0]).eval()
        m.load_state_dict(NR.fill_state({k: tuple(v.shape) for k, v in m.state_dict().items()}, 40))
        return m.to(DEV)

    m = make()
    xs = [x.to(DEV) for x in NR.make_inputs(41, NR.LSS["images"], NR.LSS["channels"], NR.LSS["maps"], relu=True)]
    with torch.no_grad():
        assert m.hip_route(xs)
        old = m(xs).clone()                                 # packs cached on the weights before the step
    opt = O.FusedAdamW(m.parameters(), lr=1e-2, grad_clip=OR.CLIP)
    g = torch.Generator().manual_seed(42)
    for p in m.parameters():
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    opt.step()
    fresh = make()
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        got, want = m(xs), fresh(xs)
    assert torch.equal(got, want) and not torch.equal(got, old)


def test_captured_step_equals_eager_steps():
    case = OR.make_case(SEED, 1.0)
    lrs = [1.0, 0.5, 0.25]                                  # the scheduler's factor per step

    def schedule(opt, s):
        for i, g in enumerate(opt.param_groups):
            g["lr"] = OR.hyper(i)[0] * lrs[s]
        opt.sync_hyper()

    ps_e, eager = fused(case)
    for s in range(OR.STEPS):
        OR.set_grads(ps_e, case["grads"][s])
        schedule(eager, s)
        eager.step()
    want = OR.snapshot(eager, ps_e)

    ps, opt = fused(case)
    OR.set_grads(ps, case["grads"][0])                      # the fixed gradient buffers (one of them misaligned)
    bufs = [p.grad for p in ps[:len(OR.SIZES)]]
    schedule(opt, 0)
    opt.prepare()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        opt.step()
    for s in range(OR.STEPS):
        for b, g in zip(bufs, case["grads"][s]):
            b.copy_(g)
        schedule(opt, s)
        graph.replay()
    opt.mark_updated()
    torch.cuda.synchronize()
    got = OR.snapshot(opt, ps)
    assert got["step"] == want["step"] == [float(OR.STEPS)] * len(OR.SIZES) + [None, None]
    for k in ("p", "m", "v"):
        for i, (x, y) in enumerate(zip(got[k], want[k])):
            assert (x is None and y is None) or torch.equal(OR.bits(x), OR.bits(y)), f"{k} of tensor {i}: replay and eager differ"
    assert torch.equal(OR.bits(opt.grad_norm), OR.bits(eager.grad_norm))


def test_refusals():
    with pytest.raises(ValueError, match="contiguous"):
        O.FusedAdamW([nn.Parameter(torch.zeros(4, 6, device=DEV).t())])
    with pytest.raises(ValueError, match="float32"):
        O.FusedAdamW([nn.Parameter(torch.zeros(4, device=DEV, dtype=torch.float16))])
    with pytest.raises(NotImplementedError, match="norm_type"):
        O.FusedAdamW([nn.Parameter(torch.zeros(4, device=DEV))], grad_clip=dict(max_norm=35, norm_type=1))
    p = nn.Parameter(torch.zeros(4, 6, device=DEV))
    opt = O.FusedAdamW([p])
    p.grad = torch.zeros(6, 4, device=DEV).t()
    with pytest.raises(ValueError, match="gradient"):
        opt.step()
    assert _lib.lib().rac_adamw_step(None, 1, None, 1, None, None, None, None, None, 1.0, _lib.OPT_ALL, None) == -1
