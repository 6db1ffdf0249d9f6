"""The float64 criterion for the AdaptiveMixing forward kernels (rac_mixing_fwd / rac_mixing_period_fwd: mixing_c64_kernel and
mixing_c64_f16x3_kernel of csrc/mixing.hip): cases, references, magnitudes, restatements and negative controls, shared by
tests/test_mixing_fwd_f64_cpu.py and tests/test_mixing_fwd_f64_gpu.py (test helper, no GPU).

The thing under test is a ``runner``: an object with
  dev(t) / host(t)                      a CPU tensor onto the runner's device and back
  mixing(x, params, P, G, **kw)         racformer_amd.fused.mixing_fused's keywords split, param_scale, f16x3, out, period -> out
``Restated`` is the runner of the CPU module: the float32 restatement of the core for the f32 mode and a model of the
split-precision arithmetic for the f16x3 mode; with ``fault=`` it is each of the negative controls (FAULTS).

Per (query, group) item, LayerNorm over the whole tile, no affine, biased variance, eps 1e-5 (tests/mixing_ref.py):
    A = x M [P,64],  A^ = LN(A),  Y = relu(A^);   B = S Y [128,64],  B^ = LN(B),  Z = relu(B^),   M, S = params * param_scale.

Reference: mixing_ref.forward64 on the float32 inputs, the parameters multiplied by param_scale in float64.
Magnitude A, per element: the same chain with every term non-negative, as mixing_ref.reference_with_scales builds it --
A_A = |x||M|, A_A^ from _ln_scale, Y carries A_A^ unmasked (ReLU is 1-Lipschitz: no margin from the kinks, no redrawing),
A_B = |S|(Y + A_Y), A_Z = A_B^ unmasked.

Criterion, f32 mode, per element:   |got - ref| <= max(4 * E_ref, 1) * 2^-24 * A
E_ref the float32 torch restatement's own worst err / A on the same case; an element with A == 0 is exactly 0; NaN exactly
where float64 has NaN.

Criterion, f16x3 mode:   |got - ref| <= max(4 * E_ref, 1) * 2^-24 * A + R
R is what the kernel's operand representation (header of the split-precision section of mixing.hip) gives away before any
arithmetic is done, pushed to first order through the same chain.  Derivation, absolute perturbations throughout:
  * x @ M: x and M * param_scale are three bf16 terms each (8 significant bits a term, 24 in all: exact) and the products
    t_i u_j with i + j <= 4 are kept.  The dropped ones are t2 u3, t3 u2 (each at most 2^-8 * 2^-16 of |x||M|) and t3 u3:
        dA = 2^-23 |x||M|                                                                     (the header's "truncation 2^-23")
  * LayerNorm: dA^ = r1 (dA + mean dA) + |A^| r1^2 mean(|A - mean A| (dA + mean dA)) -- _ln_scale with own = 0: the mean's and
    the variance's first-order answers to dA, without the roundings of r1 itself (those are the 2^-24 * A term's).
  * Y = hi + lo, two f16 (round to nearest): |Y - hi| <= 2^-11 |Y|, |Y - hi - lo| <= 2^-11 |Y - hi| -- unless lo is an f16
    subnormal, whose quantum is 2^-24:       dY = dA^ + max(2^-22 Y, 2^-25)              (ReLU passes dA^ on at most unchanged)
  * S * param_scale likewise, split as it is (no scale of its own):
        dS = max(2^-22 |S|, 2^-25)                  ("fixed", what is asserted;  "none": without the floor, reported beside it)
  * the dropped lo * lo product: at most 2^-11 |S| * 2^-11 Y, so
        dB = |S| dY + dS Y + 2^-22 |S| Y
  * R = dB^ from dB as dA^ from dA.
R is derived, not fitted: nothing in it was chosen after looking at the kernel's error.

Cases (CASES): N x G items, N in 3..6, G in {1, 4}, every item with contents of its own (a wrong item index shows, the f16x3
kernel's reversed walk included); P over every count of live 16-row tiles, both sides of every float4 / 32-block boundary of
an S row; statistics items (x = 0, eps-dominated, offset 1e3, outlier, groups scaled 1 / 3e5 / 1e-6 / 40) beside ordinary
ones; param_scale 2^-6; params as a column slice of wider rows; period N/2 and 1; out as a middle row range of a NaN-filled
buffer; the split image of each mode at P in {7, 96}; poisoned items; and the f16x3 sweep of std(S) = 2^-12 .. 2^4.

The floor of dS is the kernel's known limit.  Below |S| = 2^-3 the lo half of S is an f16 subnormal, S carries an absolute error of
2^-25 whatever its size, and the second LayerNorm brings B back to O(1): the sweep records, beside the asserted figure, err over
what the criterion allows with the floor taken out of R ("ratio_without_floor") -- above 1 from std(S) = 2^-8 down at P = 7 and at
2^-12 at P = 96 (the model here and the MI355X agree to three digits).  A per-item power-of-two scale of S removes the floor; it was
measured and left out for its cost (profiles/mixing_fwd_s_scale_ab.json)."""
import functools
import math

import torch

import mixing_ref as MR
from rowwise_ref import RATIO, TINY, U, OutOfBound, bits_equal, bound_of

EPS = MR.EPS
NAN = float("nan")
F32, F64 = torch.float32, torch.float64
SPLIT_ACT_SCALE = 16.0
OUT, C = 128, 64
P_LIST = (1, 2, 3, 4, 5, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65, 93, 95, 96)
SWEEP_K = tuple(range(-12, 5, 2))
MODES = ("f32", "f16x3")
GROUP_SCALES = (1.0, 3.0e5, 1.0e-6, 40.0)


# ------------------------------------------------------------------------------------------------------------------ cases
def _cases():
    c = {}
    for i, P in enumerate(P_LIST):
        c[f"P{P}"] = dict(N=3 + i % 4, G=(1, 4)[i % 2], P=P, guard=i % 3 != 2)
    for P in (96, 7):
        for ps in (1.0, 2.0 ** -6):
            c[f"stats P{P} ps{ps:g}"] = dict(N=6, G=4, P=P, ps=ps, stats=True)
        c[f"wide rows P{P}"] = dict(N=4, G=(4, 1)[P == 7], P=P, ld=12, ps=(1.0, 2.0 ** -6)[P == 7])
        c[f"period half P{P}"] = dict(N=6, G=(1, 4)[P == 7], P=P, period=3)
        c[f"period 1 P{P}"] = dict(N=4, G=(4, 1)[P == 7], P=P, period=1)
        c[f"poison P{P}"] = dict(N=6, G=4, P=P, poison=True)
    c["wide rows P5"] = dict(N=3, G=4, P=5, ld=2048)
    for P in (96, 7):
        for k in SWEEP_K:
            c[f"sweep k{k} P{P}"] = dict(N=3, G=1, P=P, s_std=2.0 ** k, guard=False)
    return c


CASES = _cases()
PLAIN = [n for n, s in CASES.items() if not s.get("poison") and "s_std" not in s]
POISON = [n for n, s in CASES.items() if s.get("poison")]
SWEEP = [n for n, s in CASES.items() if "s_std" in s]
# (item, group) of the statistics items; items 0 and 5 are ordinary, their four groups scaled by GROUP_SCALES
STAT_ITEMS = {"zero": (1, 0), "eps": (2, 1), "offset": (3, 2), "outlier": (4, 3)}
POISON_ITEMS = {"nan in x": (1, 0), "inf in x": (2, 1), "nan in M": (3, 2), "nan in S": (4, 3)}


@functools.lru_cache(maxsize=None)
def build(name):
    """-> the case: x [1,N,G,P,64], params [1,rows,width] (a column slice of ``wide`` [1,rows,ld]), rows = period; read-only"""
    s = CASES[name]
    N, G, P = s["N"], s["G"], s["P"]
    ps, period = s.get("ps", 1.0), s.get("period", N)
    g = torch.Generator().manual_seed(7000 + list(CASES).index(name))
    x = torch.randn(1, N, G, P, C, generator=g)
    per = C * C + OUT * P
    par = torch.empty(period, G, per)
    par[..., :C * C] = torch.randn(period, G, C * C, generator=g) * 0.3
    par[..., C * C:] = torch.randn(period, G, OUT * P, generator=g) * s.get("s_std", 0.5)
    M, S = par[..., :C * C].view(period, G, C, C), par[..., C * C:].view(period, G, OUT, P)
    if s.get("stats"):
        for n in (0, 5):
            x[0, n] *= torch.tensor(GROUP_SCALES).view(G, 1, 1)
        n, gr = STAT_ITEMS["zero"]
        x[0, n, gr] = 0
        # A = x M has std 2.4 std(x): var(A) = 1e-5.  ReLU and the second LayerNorm pass a common factor of Y on unchanged, so what
        # the first eps does shows in Z only through the second: S of this item is small enough for var(B) = 1e-5 as well
        n, gr = STAT_ITEMS["eps"]
        x[0, n, gr] *= 1.3e-3
        S[n, gr] *= 1.0e-3
        n, gr = STAT_ITEMS["offset"]                   # A = 1e3 + the other 63 channels' sum (spread 1)
        x[0, n, gr, :, 1:] *= 0.4
        x[0, n, gr, :, 0] = 1.0
        M[n, gr, 0, :] = 1.0e3
        n, gr = STAT_ITEMS["outlier"]
        x[0, n, gr, P // 2, 37] = 1.0e4
    clean = None
    if s.get("poison"):
        clean = (x.clone(), par.clone().view(1, period, G * per))
        n, gr = POISON_ITEMS["nan in x"]
        x[0, n, gr, P - 1, 5] = NAN
        n, gr = POISON_ITEMS["inf in x"]
        x[0, n, gr, 0, 63] = math.inf
        n, gr = POISON_ITEMS["nan in M"]
        M[n, gr, 63, 17] = NAN
        n, gr = POISON_ITEMS["nan in S"]               # the last valid column: the ragged tail of the staged row
        S[n, gr, 77, P - 1] = NAN
    par = par / ps                                     # pre-multiplied by the inverse (a power of two: exact)
    width = G * per
    pad = s.get("ld", 0)
    wide = torch.randn(1, period, width + pad, generator=g)
    off = pad - 4 if pad else 0
    wide[0, :, off:off + width] = par.view(period, width)
    return dict(name=name, N=N, G=G, P=P, ps=ps, period=period, x=x, wide=wide, off=off, width=width, params=wide[..., off:off + width],
                guard=s.get("guard", True), clean=clean, poisoned=sorted(POISON_ITEMS.values()) if s.get("poison") else [],
                sweep="s_std" in s)


# ----------------------------------------------------------------------------------------- host forms of the kernels' helpers
def split_f16(v):
    """rac_split_f16: f32 -> (hi, lo), both f16, round to nearest"""
    v = v.float()
    hi = v.half()
    return hi, (v - hi.float()).half()


def split_bf16(v):
    """mix_split_bf16: f32 -> three bf16 terms (as float32 tensors)"""
    v = v.float()
    t1 = v.bfloat16().float()
    r1 = v - t1
    t2 = r1.bfloat16().float()
    return t1, t2, (r1 - t2).bfloat16().float()


def split_image(z):
    """the line image of out * SPLIT_ACT_SCALE: z [N, K] f32 -> [N, K/32, hi 32 | lo 32] f16"""
    hi, lo = split_f16(z.float() * SPLIT_ACT_SCALE)
    n = z.shape[0]
    return torch.cat([hi.view(n, -1, 32), lo.view(n, -1, 32)], -1)


def image_equal(a, b):
    """bit for bit, except that any NaN matches any NaN"""
    a, b = a.contiguous(), b.contiguous()
    same = (a.view(torch.int16) == b.view(torch.int16)) | (torch.isnan(a) & torch.isnan(b))
    return a.shape == b.shape and bool(same.all())


# --------------------------------------------------------------------------------------------------------- restatements
FAULTS = ("ln1_over_padded_rows", "s_last_column_dropped", "param_row_q_div_period", "group_offset_with_P96", "unbiased_variance",
          "eps_dropped", "param_scale_not_on_M", "hi_lo_dropped", "relu_drops_nan")


def operands(x, params, P, G, ps, period, dtype, fault=None):
    """x [1,N,G,P,64], params [1,period,width] -> x [N,G,P,64], M [N,G,64,64], S [N,G,128,P] in ``dtype``, M and S times ps"""
    N = x.shape[1]
    per = C * C + OUT * P
    rows = params.reshape(period, G * per)
    q = torch.arange(N)
    rows = rows[q // period if fault == "param_row_q_div_period" else q % period]
    if fault == "group_offset_with_P96":               # (indices past the row wrap: the control reads other parameters, in bounds)
        idx = (torch.arange(G)[:, None] * (C * C + OUT * 96) + torch.arange(per)[None, :]) % (G * per)
        p = rows[:, idx]
    else:
        p = rows.reshape(N, G, per)
    M_raw, S_raw = p[..., :C * C].reshape(N, G, C, C), p[..., C * C:].reshape(N, G, OUT, P)
    if fault == "s_last_column_dropped":
        S_raw = S_raw.clone()
        S_raw[..., P - 1] = 0
    scale = torch.tensor(ps, dtype=dtype)
    M = M_raw.to(dtype) * (1 if fault == "param_scale_not_on_M" else scale)
    return x.to(dtype).reshape(N, G, P, C), M, S_raw.to(dtype) * scale


def layer_norm(t, rows, fault=None):
    """LayerNorm of the [rows, 64] tile in t's dtype; the first one's fault: its statistics over the 96 rows the kernel pads to"""
    n = rows * C
    if fault == "ln1_over_padded_rows":
        n = 96 * C
        mu = t.sum(dim=(-2, -1), keepdim=True) / n
        ss = ((t - mu) ** 2).sum(dim=(-2, -1), keepdim=True) + (96 - rows) * C * mu * mu
    else:
        mu = t.sum(dim=(-2, -1), keepdim=True) / n
        ss = ((t - mu) ** 2).sum(dim=(-2, -1), keepdim=True)
    var = ss / (n - 1 if fault == "unbiased_variance" else n)
    return (t - mu) * (1.0 / torch.sqrt(var + (0.0 if fault == "eps_dropped" else EPS)))


def relu(t, fault=None):
    y = torch.relu(t)
    return torch.where(torch.isnan(t), torch.zeros_like(t), y) if fault == "relu_drops_nan" else y


def restated32(x, params, P, G, ps=1.0, period=None, fault=None):
    """the core in float32 torch -> Z [N,G,128,64]"""
    xx, M, S = operands(x, params, P, G, ps, period or x.shape[1], F32, fault)
    Y = relu(layer_norm(xx @ M, P, fault), fault)
    return relu(layer_norm(S @ Y, OUT, fault if fault != "ln1_over_padded_rows" else None), fault)


def model_f16x3(x, params, P, G, ps=1.0, period=None, fault=None):
    """the f16x3 kernel's operand handling, its kept products accumulated exactly (float64) and rounded once -> Z [N,G,128,64]:
    three bf16 terms of x and of M * ps with the six products t_i u_j, i + j <= 4; f16 hi / lo of S * ps and of Y with
    hi hi + hi lo + lo hi; both LayerNorms in float32"""
    xx, M, S, = operands(x, params, P, G, ps, period or x.shape[1], F32, fault)
    xt, mt = [t.double() for t in split_bf16(xx)], [t.double() for t in split_bf16(M)]
    A = sum(xt[i] @ mt[j] for i in range(3) for j in range(3) if i + j <= 2).float()
    Y = relu(layer_norm(A, P, fault), fault)
    sh, sl = (t.double() for t in split_f16(S))
    yh, yl = (t.double() for t in split_f16(Y))
    Bm = sl @ yh + sh @ yh
    if fault != "hi_lo_dropped":
        Bm = Bm + sh @ yl
    return relu(layer_norm(Bm.float(), OUT, fault if fault != "ln1_over_padded_rows" else None), fault)


class Restated:
    """the runner of the CPU module; ``fault``: one of FAULTS, the deliberately wrong variant of a negative control"""

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault

    def dev(self, t):
        return t

    def host(self, t):
        return t

    def mixing(self, x, params, P, G, split=False, param_scale=1.0, f16x3=False, out=None, period=None):
        z = (model_f16x3 if f16x3 else restated32)(x, params, P, G, param_scale, period, self.fault)
        z = z.reshape(x.shape[1], -1)
        res = split_image(z) if split else z.view(1, *z.shape)
        if out is None:
            return res
        out.copy_(res)
        return out


# ------------------------------------------------------------------------------------- reference, magnitude, representation
def _clean(t):
    return torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> Z (float64), A, the float32 restatement's Z and R for each floor of dS, all [N,G,128,64]; read-only"""
    c = build(name)
    N, G, P, ps = c["N"], c["G"], c["P"], c["ps"]
    with torch.no_grad():
        rows = c["params"].reshape(c["period"], c["width"])[torch.arange(N) % c["period"]]
        f = MR.forward64(c["x"], (rows.double() * ps).view(1, N, c["width"]), P, G)
        ax, aM, aS = f["x"].abs(), f["M"].abs(), f["S"].abs()
        AA = ax @ aM
        AY, _ = MR._ln_scale(f["A"], AA, f["Ah"], f["r1"])
        AB = aS @ (f["Y"] + AY)
        A, _ = MR._ln_scale(f["B"], AB, f["Bh"], f["r2"])
        dAh, _ = MR._ln_scale(f["A"], 2.0 ** -23 * AA, f["Ah"], f["r1"], own=0.0)
        dY = dAh + torch.clamp(2.0 ** -22 * f["Y"], min=2.0 ** -25)
        R = {}
        for kind, floor in (("fixed", 2.0 ** -25), ("none", 0.0)):
            dS = torch.clamp(2.0 ** -22 * aS, min=floor)
            dB = aS @ dY + dS @ f["Y"] + 2.0 ** -22 * (aS @ f["Y"])
            R[kind] = MR._ln_scale(f["B"], dB, f["Bh"], f["r2"], own=0.0)[0]
        r32 = restated32(c["x"], c["params"], P, G, ps, c["period"])
    nan = torch.isnan(f["Z"])
    # (a poisoned item is NaN throughout: its magnitudes are never read)
    return dict(Z=f["Z"], A=torch.where(nan, torch.zeros_like(A), A), r32=r32, nan=nan,
                R={k: torch.where(nan, torch.zeros_like(v), v) for k, v in R.items()})


# ------------------------------------------------------------------------------------------------------------- the metric
class Log:
    """every (E_ref, kernel, allowed) triple of a session, keyed "<mode> | <case> | <output>", in units of 2^-24 of A: E_ref the
    float32 restatement's worst err / A, kernel the worst err / A of the thing under test, allowed what the criterion grants at
    that element (max(4 E_ref, 1) + R / (2^-24 A)), ratio the worst err / allowed over all elements; *_of_max_out the worst absolute
    errors in units of 2^-24 of the case's largest |Z| (reported only); ``compare`` prints, then asserts"""

    def __init__(self):
        self.errors = {}

    def compare(self, key, got, ref, A, r32, R=None, items=None, reported=None):
        """``reported``: name -> another R (or None for none at all); the worst err / allowed with it is recorded as ratio_<name>"""
        got, ref, A, r32 = (t.detach().double() for t in (got, ref, A, r32))
        R = torch.zeros_like(A) if R is None else R.double()
        reported = {k: (torch.zeros_like(A) if v is None else v.double()) for k, v in (reported or {}).items()}
        assert got.shape == ref.shape == A.shape == r32.shape == R.shape, (key, got.shape, ref.shape)
        if items is not None:                          # (only these (item, group) tiles)
            got, ref, A, r32, R = (torch.stack([t[n, g] for n, g in items]) for t in (got, ref, A, r32, R))
            reported = {}
        nan = torch.isnan(ref)
        ok = ~nan
        assert bool(torch.isfinite(ref[ok]).all()) and bool(torch.isfinite(A[ok]).all()) and bool(torch.isfinite(R[ok]).all()), key
        if not torch.equal(torch.isnan(got), nan):
            raise OutOfBound(f"{key}: NaN in {int((torch.isnan(got) & ok).sum())} elements where float64 has none, "
                             f"none in {int((~torch.isnan(got) & nan).sum())} where it has")
        if not bool((got[ok & (A == 0)] == 0).all()):
            raise OutOfBound(f"{key}: an element of magnitude 0 is not exactly 0")
        live = ok & (A > 0)
        e_ref = float(((r32 - ref).abs()[live] / A[live]).max() / U) if bool(live.any()) else 0.0
        bound = bound_of(e_ref)
        err, allowed = (got - ref).abs(), bound * U * A + R
        kernel = allowed_at = ratio = 0.0
        if bool(live.any()):
            rel = torch.where(live, err / A.clamp(min=TINY), torch.zeros_like(err)) / U
            i = int(rel.argmax())
            kernel, allowed_at = float(rel.flatten()[i]), float((allowed / (U * A.clamp(min=TINY))).flatten()[i])
            ratio = float(torch.where(live, err / allowed.clamp(min=TINY), torch.zeros_like(err)).max())
        # (the same two errors against the output's own size instead of A, which is some hundred times larger: for the reader)
        zmax = float(ref[ok].abs().max()) if bool(ok.any()) else 0.0
        e_out, k_out = ((float(t[ok].max()) / (U * zmax) if zmax > 0 else 0.0) for t in ((r32 - ref).abs(), err))
        self.errors[key] = dict(E_ref=e_ref, kernel=kernel, allowed=allowed_at, ratio=ratio, E_ref_of_max_out=e_out, kernel_of_max_out=k_out)
        for k, Ralt in reported.items():
            alt = float(torch.where(live, err / (bound * U * A + Ralt).clamp(min=TINY), torch.zeros_like(err)).max()) if bool(live.any()) else 0.0
            self.errors[key][f"ratio_{k}"] = alt
            print(f"    err / allowed with R {k.replace('_', ' ')}: {alt:.3g}")
        print(f"{key}: E_ref {e_ref:.3g}, kernel {kernel:.3g} (allowed there {allowed_at:.3g}) x 2^-24; worst err / allowed {ratio:.3g}")
        bad = ok & ~(err <= allowed + TINY)
        if bool(bad.any()):
            raise OutOfBound(f"{key}: {int(bad.sum())} elements above max({RATIO:g} x E_ref {e_ref:.3g}, 1) x 2^-24 x A"
                             f"{' + R' if bool((R > 0).any()) else ''}; worst err / allowed {ratio:.3g}")
        return bound

    def worst(self):
        """group -> the session's worst E_ref, kernel figure and err / allowed; groups: the two modes, and per mode the sweep"""
        out = {}
        for key, e in self.errors.items():
            mode, case = key.split(" | ")[:2]
            w = out.setdefault(f"{mode} sweep" if case.startswith("sweep") else mode,
                               dict(E_ref=0.0, kernel=0.0, ratio=0.0, E_ref_of_max_out=0.0, kernel_of_max_out=0.0))
            for k in e:
                if k != "allowed":
                    w[k] = max(w.get(k, 0.0), e[k])
        return out


# ------------------------------------------------------------------------------------------------------------- the checks
def launch(run, c, mode, split=False, clean=False):
    """one launch of the case -> the output on the host ([N,G,128,64] f32, or the image [N, G*256, 64] f16); with c["guard"] the
    destination is a middle row range of a NaN-filled buffer, whose other rows must still be NaN afterwards"""
    N, G, P = c["N"], c["G"], c["P"]
    x = c["clean"][0] if clean else c["x"]
    params = run.dev(c["clean"][1]) if clean else run.dev(c["wide"])[..., c["off"]:c["off"] + c["width"]]
    full = out = None
    if c["guard"]:
        full = run.dev(torch.full((N + 5, G * 256, 64), NAN, dtype=torch.float16) if split else torch.full((1, N + 5, G * OUT * C), NAN))
        out = full[2:2 + N] if split else full[:, 2:2 + N]
    res = run.mixing(run.dev(x), params, P, G, split=split, param_scale=c["ps"], f16x3=mode == "f16x3", out=out,
                     period=None if c["period"] == N else c["period"])
    if full is not None:
        full = run.host(full)
        rows = full if split else full[0]
        assert bool(torch.isnan(rows[:2]).all()) and bool(torch.isnan(rows[2 + N:]).all()), "mixing wrote outside its row range"
        res = rows[2:2 + N]
    else:
        res = run.host(res)
    want = (N, G * 256, 64) if split else (N, G * OUT * C)
    assert tuple(res.reshape(want).shape) == want and res.dtype == (torch.float16 if split else F32)
    return res.reshape(want) if split else res.reshape(N, G, OUT, C)


def check_case(log, name, run, mode, s_floor="fixed", items=None):
    """one case in one mode against float64; at P in {7, 96} the mode's split image as well.  A sweep case also records what
    the f16x3 kernel's error comes to with the floor taken out of R and with no R at all (the f32 mode's criterion)."""
    c, ref = build(name), reference(name)
    z = launch(run, c, mode)
    reported = dict(without_floor=ref["R"]["none"], absent=None) if c["sweep"] else None
    log.compare(f"{mode} | {name} | out", z, ref["Z"], ref["A"], ref["r32"], ref["R"][s_floor] if mode == "f16x3" else None, items, reported)
    if c["P"] in (7, 96) and not c["sweep"] and items is None:
        img = launch(run, c, mode, split=True)
        assert image_equal(img, split_image(z.reshape(c["N"], -1))), f"{mode} | {name}: the split image is not the split of the fp32 output"
    return z


def check_poison(log, name, run, mode):
    """NaN exactly where float64 has it, the other items bit-equal to the launch without the poison, the image non-finite in
    every line of a poisoned item and the split of the fp32 output elsewhere"""
    c, ref = build(name), reference(name)
    N, G = c["N"], c["G"]
    assert all(bool(ref["nan"][n, g].all()) for n, g in c["poisoned"]) and int(ref["nan"].sum()) == len(c["poisoned"]) * OUT * C
    z = launch(run, c, mode)
    log.compare(f"{mode} | {name} | out", z, ref["Z"], ref["A"], ref["r32"], ref["R"]["fixed"] if mode == "f16x3" else None)
    z_clean = launch(run, c, mode, clean=True)
    others = [(n, g) for n in range(N) for g in range(G) if (n, g) not in c["poisoned"]]
    assert all(bits_equal(z[n, g], z_clean[n, g]) for n, g in others), f"{mode} | {name}: an item beside a poisoned one changed"
    img = launch(run, c, mode, split=True).view(N, G, 256, 64)
    want = split_image(z.reshape(N, -1)).view(N, G, 256, 64)
    for n, g in c["poisoned"]:
        assert bool((~torch.isfinite(img[n, g])).any(-1).all()), f"{mode} | {name}: a finite line in the image of poisoned item {(n, g)}"
    assert all(bits_equal(img[n, g], want[n, g]) for n, g in others), f"{mode} | {name}: the split image beside a poisoned item"
