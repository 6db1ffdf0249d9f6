"""The AdaptiveMixing forward kernels on the MI355X against float64, element by element: rac_mixing_fwd and rac_mixing_period_fwd
(mixing_c64_kernel and mixing_c64_f16x3_kernel of csrc/mixing.hip) through racformer_amd.fused.mixing_fused.
tests/mixing_fwd_ref.py holds the cases, the reference, the magnitudes, the derivation of the representation term R and the
restatements; tests/test_mixing_fwd_f64_cpu.py runs the same checks on the CPU with the restatements in the kernels' place, shows
that each negative control fails its check, and holds the refusals that need no device.

Criterion, per element: f32 mode |got - ref| <= max(4 x E_ref, 1) x 2^-24 x A; f16x3 mode the same plus R.  ref: float64 on the
float32 inputs; E_ref: the float32 torch restatement's own worst err / A on the same case; A: the chain with every term
non-negative; an element with A == 0 is exactly 0; NaN exactly where float64 has NaN.  The split image of either mode is bit-equal
to the host split of that mode's fp32 output x SPLIT_ACT_SCALE; a destination handed in is a middle row range of a NaN-filled
buffer whose other rows must still be NaN.  Every comparison prints its (E_ref, kernel, allowed) triple; with
RAC_MIXING_FWD_ERRORS=<file> the session's triples are written there as JSON (profiles/mixing_fwd_f64.json is the MI355X run's
copy).  One launch per case and output kind, three for a poisoned case (with the poison, without it, the image).

Measured on the MI355X (80 tests in 3.0 s), worst over the session in units of 2^-24 x A (E_ref | kernel), and the worst err over
what the criterion allows:
  f32          0.43 | 0.43   0.25 of the allowance: the kernel errs as the float32 restatement does (statistics cases; the plain
                             P cases 0.03 .. 0.19 | 0.03 .. 0.17)
  f16x3        0.43 | 33     0.51 of the allowance, in the statistics cases at P = 7 on elements whose allowance is R's 2^-25 floor for
                             S (the eps-dominated item's S is 5e-4); 0.17 at P = 96; the plain P cases 0.03 .. 0.19 | 0.03 .. 0.17, at
                             most 0.053 of the allowance
  split images bit-equal to the host split of the mode's own fp32 output x 16 in all 14 cases x 2 modes with P in {7, 96} (no figure)
  sweep        0.14 | 45     0.51 of the allowance (std(S) = 2^-12, P = 7); per std(S) = 2^k, kernel err / allowed with R as asserted,
                             with the 2^-25 floor of S taken out of R, and the kernel's | the restatement's error in 2^-24 of the
                             largest output:
                 k     P = 96: asserted  no floor   of output      P = 7: asserted  no floor   of output
                -12            0.18      3.3       1094 | 5.5             0.51      14.8        868 | 4.0
                -10            0.13      0.68       245 | 5.8             0.46       3.8        221 | 4.0
                 -8            0.09      0.20        76 | 5.9             0.33       1.04        56 | 3.8
                 -6            0.05      0.07        19 | 5.1             0.15       0.22        17 | 3.7
                 -4            0.01      0.01       5.2 | 4.9             0.06       0.07       4.4 | 3.7
              -2 .. 4         <0.01     <0.01   3.7-4.5 | 5.2-5.7        <0.03      <0.03   3.2-4.3 | 3.3-4.2
No comparison is at its limit.  A is some hundred times the output (the second LayerNorm's scale counts every term of B at full
size), so E_ref is small and the floor of 1 x 2^-24 x A is what binds in the plain cases; the last two columns are there for that.
The sweep shows the f16x3 kernel's known limit: S is split with no scale of its own, its lo half is a subnormal below |S| = 2^-3, and
the kernel leaves fp32 grade below std(S) = 2^-6 (by the criterion without the floor: from 2^-8 down at P = 7, at 2^-12 at P = 96).
The per-item scale that removes it cost 1.0 us of 83.5 us per f8 launch against a spread of 0.2 us and was left out
(profiles/mixing_fwd_s_scale_ab.json): R keeps its floor and the kernel is asserted to be as accurate as its
representation allows.

Found by this module and fixed with it: all five ReLUs of mixing.hip were fmaxf(v, 0), which turns a NaN into 0.  Before, on the
parent's kernels: "poison P7" and "poison P96" in both modes each had "NaN in 0 elements where float64 has none, none in 32768
where it has" -- the four poisoned items (NaN in x, +inf in x, NaN in M, NaN in the last valid column of S) came out as 8192 exact
zeros each.  After (rac_relu in the f32 forward and the backward's recompute, mix_relu_ln in the f16x3 kernel): all four tests pass,
each poisoned item is NaN throughout in the fp32 output and in every line of the image, every other item has the bits of the
launch without the poison, and the f16x3 image of the f8 launch is bit-identical to the parent's; golden, parity, mixing_grad and
layer0_once tests untouched and green.
"""
import json
import os

import pytest
import torch

import mixing_fwd_ref as W
from racformer_amd import fused

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Kernels:
    """the runner of tests/mixing_fwd_ref.py on the device, through the public wrapper"""

    def dev(self, t):
        return t.to(DEV)

    def host(self, t):
        torch.cuda.synchronize()
        return t.cpu()

    def mixing(self, x, params, P, G, **kw):
        return fused.mixing_fused(x, params, P, G, 128, W.EPS, **kw)


RUN = Kernels()


@pytest.fixture(scope="module")
def log():
    n = torch.get_num_threads()
    torch.set_num_threads(min(n, 16))
    lg = W.Log()
    yield lg
    torch.set_num_threads(n)
    worst = lg.worst()
    print("\nAdaptiveMixing forward against float64, worst per group in units of 2^-24 (E_ref | kernel | err / allowed):")
    for k in sorted(worst):
        print(f"  {k:>12s}: {worst[k]['E_ref']:8.4f} | {worst[k]['kernel']:8.4f} | {worst[k]['ratio']:.4f}")
    path = os.environ.get("RAC_MIXING_FWD_ERRORS")
    if lg.errors and path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(dict(unit="2**-24", ratio_allowed=W.RATIO, floor=1.0, s_floor_of_R=2.0 ** -25, worst=worst, errors=lg.errors), f,
                      indent=1, sort_keys=True)


@pytest.mark.parametrize("mode", W.MODES)
@pytest.mark.parametrize("name", W.PLAIN)
def test_case(log, name, mode):
    W.check_case(log, name, RUN, mode)


@pytest.mark.parametrize("mode", W.MODES)
@pytest.mark.parametrize("name", W.POISON)
def test_poisoned_items(log, name, mode):
    """a NaN or inf in an item's x, M or S: that item is NaN where float64's is (all 8192 outputs), in the image too, and every
    other item of the launch keeps its bits"""
    W.check_poison(log, name, RUN, mode)


@pytest.mark.parametrize("name", W.SWEEP)
def test_s_magnitude_sweep(log, name):
    """std(S) = 2^-12 .. 2^4 in the f16x3 mode: asserted with R as derived (the 2^-25 floor of S in it); what the error comes to
    without that floor, and without R, is recorded beside it"""
    W.check_case(log, name, RUN, "f16x3")
