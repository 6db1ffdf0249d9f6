"""The float64 criterion for the decoder's small-launch forward chain (rac_rowgemm_fwd, rac_add_ln_fwd, rac_pe_head_fwd,
rac_refine_fwd / rac_layer_boundary_fwd, rac_gru_gate_fwd, rac_upsample2x_fwd): cases, references, magnitudes, negative controls and
the launcher rules, shared by tests/test_rowwise_f64_cpu.py and tests/test_rowwise_f64_gpu.py (test helper, no GPU).

The thing under test is a ``runner``: an object with
  dev(t) / host(t)                           a CPU tensor onto the runner's device and back
  add_ln(s, out, split_out)                  -> out                          (s: a segment description on the device, see ``seg``)
  rowgemm(gemms, rows)                       writes the ``out`` / ``x_out`` / ``split_out`` views of the descriptions
  pe_head(x3, W, b, gamma, beta, eps)        -> [..., 256]
  refine(prop, delta, td)                    -> (pred, xy)
  layer_boundary(prop, delta, td, W, b, gamma, beta, eps, xy_out) -> (pred, xy, table, pe)
  box_prep(boxes)                            -> table
  gru_gate(gates, h_prev, h_out, bias_map, h_out2)
  upsample2x(x)                              -> [N,C,2h,2w]
``Restated32`` is the float32 restatement of the same functions on the CPU: it stands in for the kernels in the CPU module, gives
every comparison its E_ref in the GPU module, and -- with ``fault=`` -- is each of the negative controls (the issue's eleven and
a ReLU that drops a NaN).

Criterion, per element: |got - ref| <= max(4 * E_ref, 1) * 2^-24 * A; ref the float64 evaluation of the torch / oracle.restate
formulation on the same float32 inputs, E_ref the float32 restatement's own worst err / A on the same case, A the same expression
with every term non-negative (the magnitudes below); an element with A == 0 is exactly 0; NaN exactly where the reference has NaN.
Every destination a check hands out is a region of a larger buffer filled with a NaN sentinel (extra rows, a wider row stride,
neighbouring [:, t] slots): everything outside the region must still be the sentinel afterwards."""
import math

import torch
import torch.nn.functional as TF

from oracle import restate as R
from racformer_amd import synthetic as syn

U = 2.0 ** -24
RATIO = 4.0
TINY = 1e-30
NAN = float("nan")
FLT_MAX = float(torch.finfo(torch.float32).max)
F32, F64 = torch.float32, torch.float64
PC = list(syn.PC_RANGE)
NUM_RAY = 150
LN_EPS = 1e-5
SPLIT_SCALE, SPLIT_PAD = 16.0, 64
SIZES = (1, 3, 4, 5)                     # rows around the 4-row workgroups of the row-wise kernels


class OutOfBound(AssertionError):
    """a comparison missed the criterion (what every negative control has to raise)"""


# ------------------------------------------------------------------------------------------------------------- the metric
def bound_of(e_ref):
    return max(RATIO * e_ref, 1.0)


def figure(got, ref, A, ok):
    """worst |got - ref| / A over the compared elements with A > 0, in units of 2^-24"""
    live = ok & (A > 0)
    if not bool(live.any()):
        return 0.0
    return float(((got - ref).abs()[live] / A[live]).max() / U)


class Log:
    """every (E_ref, kernel) pair of a session, keyed "<kernel> | <case> | <output>"; ``compare`` prints the pair, then asserts"""

    def __init__(self):
        self.errors = {}

    def compare(self, key, got, ref, A, r32):
        got, ref, A, r32 = (x.detach().double() for x in (got, ref, A, r32))
        assert got.shape == ref.shape == A.shape == r32.shape, (key, got.shape, ref.shape, A.shape, r32.shape)
        nan = torch.isnan(ref)
        assert bool(torch.isfinite(ref[~nan]).all()) and bool(torch.isfinite(A[~nan]).all()), f"{key}: the reference is not finite"
        if not torch.equal(torch.isnan(got), nan):
            raise OutOfBound(f"{key}: NaN in {int((torch.isnan(got) & ~nan).sum())} elements where float64 has none, "
                             f"none in {int((~torch.isnan(got) & nan).sum())} where it has")
        ok = ~nan
        if not bool((got[ok & (A == 0)] == 0).all()):
            raise OutOfBound(f"{key}: an element of magnitude 0 is not exactly 0")
        e_ref, kernel = figure(r32, ref, A, ok), figure(got, ref, A, ok)
        bound = bound_of(e_ref)
        self.errors[key] = dict(E_ref=e_ref, kernel=kernel)
        print(f"{key}: E_ref {e_ref:.3g}, kernel {kernel:.3g} (allowed {bound:.3g}) x 2^-24")
        bad = ok & ~((got - ref).abs() <= bound * U * A + TINY)
        if not kernel <= bound or bool(bad.any()):
            raise OutOfBound(f"{key}: {kernel:.3g} above {bound:.3g} = max({RATIO:g} x E_ref {e_ref:.3g}, 1) in {int(bad.sum())} elements")
        return bound

    def worst(self):
        """kernel -> worst E_ref, kernel figure and kernel / allowed of the session"""
        out = {}
        for key, e in self.errors.items():
            w = out.setdefault(key.split(" | ")[0], dict(E_ref=0.0, kernel=0.0, worst_ratio=0.0))
            w["E_ref"], w["kernel"] = max(w["E_ref"], e["E_ref"]), max(w["kernel"], e["kernel"])
            w["worst_ratio"] = max(w["worst_ratio"], e["kernel"] / bound_of(e["E_ref"]))
        return out


def bits_equal(a, b):
    """bit for bit (NaN payloads included)"""
    it = {torch.float32: torch.int32, torch.float16: torch.int16}[a.dtype]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(it), b.contiguous().view(it))


# ------------------------------------------------------------------------------------------------------- guarded buffers
def guard(rows, width, ld=None, off=None, extra=2, dtype=F32):
    """-> (a [rows + extra, ld] buffer of NaN, the [rows, width] region a kernel may write)"""
    if ld is None:
        ld, off = (width + 3) // 4 * 4 + 8, 4
    full = torch.full((rows + extra, ld), NAN, dtype=dtype)
    return full, (slice(0, rows), slice(off, off + width))


def guard_image(rows, width):
    """split images are contiguous: extra rows only"""
    return torch.full((rows + 2, width), NAN, dtype=torch.float16), (slice(0, rows), slice(0, width))


def taken(full, region):
    """the region's content, after asserting that everything outside it still is the sentinel"""
    outside = torch.ones(full.shape, dtype=torch.bool)
    outside[region] = False
    assert bool(torch.isnan(full[outside]).all()), "a kernel wrote outside its destination"
    return full[region]


# ------------------------------------------------------------------------------------------------ prologue / LayerNorm rows
def layer_norm(x, gamma, beta, eps, fault=None):
    if fault is None:
        return TF.layer_norm(x, x.shape[-1:], gamma.to(x.dtype), beta.to(x.dtype), eps)
    dim = x.shape[-1]
    d = x - x.mean(-1, keepdim=True)
    var = (d * d).sum(-1, keepdim=True) / (dim - 1 if fault == "variance_over_dim_minus_1" else dim)
    return d / torch.sqrt(var + (0.0 if fault == "eps_dropped" else eps)) * gamma.to(x.dtype) + beta.to(x.dtype)


def seg(g, rows, dim=256, P=1, scale=1.0, bias0=False, res=False, norm=False, relu=False, post=False, x_out=False, split=None, ld=None,
        x_ld=None):
    """One 256-wide segment of a row GEMM's A operand, or (any ``dim``) the operands of an add_ln launch:
    [relu](LN(scale * sum_p a[p] + bias0 + res)) [+ post].  ``ld``: the single source and the residual are column slices of
    [rows, ld] tensors; ``x_ld``: so is the destination of the finished rows."""
    r = lambda *shape: torch.randn(*shape, generator=g)                                  # noqa: E731
    s = dict(rows=rows, dim=dim, P=P, scale=scale, relu=relu, x_out=x_out, split=split, x_ld=x_ld, src={})

    def rows_of(name):
        if ld is None:
            s[name] = r(rows, dim)
        else:
            full, region = r(rows, ld), (slice(None), slice(ld - dim - 4, ld - 4))
            s["src"][name], s[name] = (full, region), full[region]
    if P > 1:
        s["a"] = r(P, rows, dim)
    else:
        rows_of("a")
    s["bias0"] = r(dim) if bias0 else None
    s["res"] = None
    if res:
        rows_of("res")
    s["gamma"], s["beta"] = (r(dim), r(dim)) if norm else (None, None)
    s["eps"] = LN_EPS
    s["post"] = r(rows, dim) if post else None
    return s


STATS = ("constant", "offset", "tiny", "outlier", "zero")


def set_row(s, row, kind):
    """one row's statistics, in place (segments without bias0 only)"""
    assert s["bias0"] is None
    a = s["a"][:, row] if s["P"] > 1 else s["a"][row]
    res = s["res"][row] if s["res"] is not None else None
    if kind == "constant":                        # LayerNorm of a constant row: exactly beta (0.5 * P and the mean are exact)
        a[...] = 0.5
    elif kind == "offset":                        # 1e4 with unit spread
        a += 1e4 / s["P"]
    elif kind == "tiny":                          # every source x 1e-4: eps dominates the variance
        a *= 1e-4
        if res is not None:
            res *= 1e-4
    elif kind == "outlier":
        a[..., 77 % s["dim"]] = 1e4
    elif kind == "zero":
        a[...] = 0
    elif kind == "nan":
        a[..., 5 % s["dim"]] = NAN
    if kind in ("constant", "zero") and res is not None:
        res[...] = 0


def pro_pre(s, dtype, fault=None):
    """the rows before the norm"""
    a = s["a"].to(dtype)
    if s["P"] > 1:
        a = (a[:-1] if fault == "partial_dropped" else a).sum(0)
    b0 = s["bias0"].to(dtype) if s["bias0"] is not None else None
    if fault == "scale_after_bias" and b0 is not None:
        x = (a + b0) * s["scale"]
    else:
        x = a * s["scale"]
        if b0 is not None:
            x = x + b0
    if s["res"] is not None:
        res = s["res"].to(dtype)
        x = x + (torch.roll(res, -1, 0) if fault == "residual_next_row" else res)
    return x


def relu(x, fault=None):
    """torch.relu keeps a NaN; the fault turns it into 0, as fmaxf(NaN, 0) does"""
    y = torch.relu(x)
    return torch.where(torch.isnan(x), torch.zeros_like(x), y) if fault == "relu_drops_nan" else y


def pro_value(s, dtype, fault=None):
    x = pro_pre(s, dtype, fault)
    if s["gamma"] is not None:
        x = layer_norm(x, s["gamma"], s["beta"], s["eps"], fault if fault in ("variance_over_dim_minus_1", "eps_dropped") else None)
    if s["relu"]:
        x = relu(x, fault)
    if s["post"] is not None:
        x = x + s["post"].to(dtype)
    return x


def ln_magnitude(X, pre64, gamma, beta, eps):
    """A_i = (X_i + mean_j X_j) * rstd64 * |gamma_i| + |beta_i|"""
    rstd = 1.0 / torch.sqrt(pre64.var(-1, unbiased=False, keepdim=True) + eps)
    return (X + X.mean(-1, keepdim=True)) * rstd * gamma.double().abs() + beta.double().abs()


def pro_mag(s):
    a = s["a"].double().abs()
    X = abs(s["scale"]) * (a.sum(0) if s["P"] > 1 else a)
    for k in ("bias0", "res"):
        if s[k] is not None:
            X = X + s[k].double().abs()
    A = ln_magnitude(X, pro_pre(s, F64), s["gamma"], s["beta"], s["eps"]) if s["gamma"] is not None else X
    return A + s["post"].double().abs() if s["post"] is not None else A


def split_image(x, layout):
    """the f16 image of float32 rows: hi = (x * 16).half(), lo = (x * 16 - hi.float()).half()"""
    rows, dim = x.shape
    xs = x.float() * SPLIT_SCALE
    hi = xs.half()
    lo = (xs - hi.float()).half()
    if layout == "lines":                          # [hi 32 | lo 32] per 32 columns
        return torch.cat([hi.view(rows, dim // 32, 32), lo.view(rows, dim // 32, 32)], -1).reshape(rows, 2 * dim)
    pad = torch.zeros(rows, SPLIT_PAD, dtype=torch.float16)
    pad[:, :2] = SPLIT_SCALE
    return torch.cat([hi, hi, lo, pad], 1)         # K-concatenated [hi | hi | lo | 16 16 0...]


def image_width(dim, layout):
    return 2 * dim if layout == "lines" else 3 * dim + SPLIT_PAD


def seg_on(run, s):
    """the description with its operands on the runner's device (column slices stay column slices)"""
    d = dict(s)
    for k in ("a", "bias0", "res", "gamma", "beta", "post"):
        if s[k] is not None:
            d[k] = run.dev(s["src"][k][0])[s["src"][k][1]] if k in s["src"] else run.dev(s[k])
    return d


def check_finished_rows(log, key, s, x, image, special=()):
    """the finished rows of one segment (x_out / add_ln's out) and the f16 image written beside them"""
    bound = log.compare(key, x, pro_value(s, F64), pro_mag(s), pro_value(s, F32))
    for row, kind in special:
        if kind in ("constant", "zero") and s["post"] is None:
            want = torch.relu(s["beta"]) if s["relu"] else s["beta"]
            assert torch.equal(x[row], want), f"{key}: the {kind} row {row} is not exactly beta"
        if kind == "nan":                          # the row is NaN, the rows beside it are not (and within the bound, above)
            assert bool(torch.isnan(x[row]).all()), f"{key}: the poisoned row {row} is not NaN throughout"
            beside = [r for r in range(row - row % 4, min(row - row % 4 + 4, x.shape[0])) if r != row]
            assert len(beside) == 3 and bool(torch.isfinite(x[beside]).all()), f"{key}: rows beside the poisoned row {row}"
    if image is not None:
        assert bits_equal(image, split_image(x, s["split"])), f"{key}: the f16 {s['split']} image is not the split of the rows written"
    return bound


# ---------------------------------------------------------------------------------------------------------------- add_ln
def add_ln_kernel(dim, S):
    """which kernel rac_add_ln_fwd launches"""
    return "many" if dim == 256 and S >= 8 else "simple"


def _add_ln_cases():
    cases = {}
    rows_of = (1, 3, 4, 5, 205)
    i = 0
    for dim in (4, 100, 256, 260, 512, 1024):
        for S in (1, 2, 7):
            lines = dim % 32 == 0 and S == 2
            cases[f"simple dim{dim} S{S}"] = dict(rows=rows_of[i % 5], dim=dim, P=S, scale=(1.0, 0.25, -1.5)[i % 3], bias0=i % 2 == 0,
                                                  res=i % 3 != 1, relu=i % 4 == 1, post=i % 3 == 0, ld=dim + 12 if S == 1 else None,
                                                  split="lines" if lines else ("kcat" if S == 7 else None), out_slice=i % 2 == 1, kernel="simple")
            i += 1
    for S in (8, 9, 13, 16, 32):
        cases[f"many dim256 S{S}"] = dict(rows=rows_of[i % 5], dim=256, P=S, scale=(1.0, 0.25, -1.5)[i % 3], bias0=i % 2 == 0, res=i % 3 != 1,
                                          relu=i % 4 == 1, post=i % 3 == 0, ld=None, split=(None, "lines", "kcat")[i % 3],
                                          out_slice=i % 2 == 1, kernel="many")
        i += 1
    for name, S in (("simple", 1), ("simple", 7), ("many", 8), ("many", 13)):
        cases[f"{name} statistics S{S}"] = dict(rows=16, dim=256, P=S, scale=1.0, bias0=False, res=S == 7, relu=False, post=False, ld=None,
                                                split=None, out_slice=True, kernel=name, stats=True)
    # a NaN row behind a ReLU stays NaN, as torch.relu keeps it
    for name, S in (("simple", 2), ("many", 9)):
        cases[f"{name} nan relu S{S}"] = dict(rows=9, dim=256, P=S, scale=1.0, bias0=False, res=True, relu=True, post=False, ld=None,
                                              split=None, out_slice=True, kernel=name, special=((5, "nan"),))
    cases["simple plain rows205"] = dict(rows=205, dim=256, P=1, scale=1.0, bias0=False, res=False, relu=False, post=False, ld=None, split=None,
                                         out_slice=False, kernel="simple")
    return cases


ADD_LN_CASES = _add_ln_cases()
# each beside ordinary rows; the NaN row with three clean rows in its 4-row workgroup of the simple kernel (rows 12 .. 15)
STAT_ROWS = tuple((1 + 2 * i, kind) for i, kind in enumerate(STATS)) + ((13, "nan"),)


def add_ln_build(name):
    c = ADD_LN_CASES[name]
    g = torch.Generator().manual_seed(1000 + list(ADD_LN_CASES).index(name))
    s = seg(g, c["rows"], c["dim"], c["P"], c["scale"], c["bias0"], c["res"], True, c["relu"], c["post"], True, c["split"], c["ld"])
    s["special"] = STAT_ROWS if c.get("stats") else c.get("special", ())
    for row, kind in s["special"]:
        set_row(s, row, kind)
    s["out_slice"] = c["out_slice"]
    return s


def check_add_ln(log, key, s, run):
    rows, dim = s["rows"], s["dim"]
    full = region = img = None
    if s["out_slice"]:
        full, region = guard(rows, dim)
        full = run.dev(full)
    if s["split"]:
        img, img_region = guard_image(rows, image_width(dim, s["split"]))
        img = run.dev(img)
    out = run.add_ln(seg_on(run, s), full[region] if full is not None else None, img[img_region] if img is not None else None)
    x = taken(run.host(full), region) if full is not None else run.host(out).reshape(rows, dim)
    image = taken(run.host(img), img_region) if img is not None else None
    return check_finished_rows(log, f"add_ln | {key} | out", s, x, image, s["special"])


# --------------------------------------------------------------------------------------------------------------- rowgemm
def rowgemm_instantiation(rows, widths, nseg):
    """(NSEG, MT, EARLY) of the rowgemm_kernel a launch takes"""
    grid = (rows + 15) // 16 * ((max(widths) + 63) // 64) * len(widths)
    return nseg, 1, not (nseg == 1 and grid > 512)


def gemm(g, segs, N, bias=True, relu_from=None, out_ld=None):
    K = sum(s["dim"] for s in segs)
    return dict(segs=segs, N=N, W=torch.randn(N, K, generator=g) / 16, b=torch.randn(N, generator=g) if bias else None,
                relu_from=relu_from, out_ld=out_ld)


def gemm_value(gm, dtype, fault=None):
    X = torch.cat([pro_value(s, dtype, fault) for s in gm["segs"]], -1)
    if fault == "k_block_dropped":
        X = X.clone()
        X[:, 16:32] = 0
    out = X @ gm["W"].to(dtype).t()
    if gm["b"] is not None:
        out = out + gm["b"].to(dtype)
    if gm["relu_from"] is not None:
        rf = gm["relu_from"] + (1 if fault == "relu_from_off_by_one" else 0)
        out = torch.cat([out[:, :rf], relu(out[:, rf:], fault)], 1)
    return out


def gemm_mag(gm):
    """A_n = sum_k A^X_k |W_nk| + |b_n|"""
    A = torch.cat([pro_mag(s) for s in gm["segs"]], -1) @ gm["W"].double().abs().t()
    return A + gm["b"].double().abs() if gm["b"] is not None else A


def _rowgemm_cases():
    """name -> (rows, [per GEMM: (N, bias, relu_from, out_ld, [segment keywords])], special rows of segment 0 of GEMM 0)"""
    plain, c = {}, {}
    xo = dict(x_out=True)
    widths = (1, 10, 63, 64, 65, 512, 2189)
    for i, rows in enumerate((1, 15, 16, 17, 37)):          # every row count with 1, 2 and 3 segments, the widths in turn
        for nseg in (1, 2, 3):
            j = 3 * i + nseg - 1
            c[f"plain r{rows} {nseg}seg N{widths[j % 7]}"] = (rows, [(widths[j % 7], j % 4 != 3, (None, 0, 7)[j % 3], None, [plain] * nseg)])
    # the decoder's prologues (transformer.py, _front and forward_fused)
    c["ln relu post xout r37 N512"] = (37, [(512, True, None, None, [dict(norm=True, relu=True, post=True, **xo)])])
    c["res ln xout lines r17 N2189"] = (17, [(2189, True, None, (2192, 0), [dict(res=True, norm=True, split="lines", **xo)])])
    c["res ln kcat r16 N64"] = (16, [(64, True, None, None, [dict(res=True, norm=True, split="kcat", **xo)])])
    c["P3 ln xout relu0 r37 N512"] = (37, [(512, True, 0, None, [dict(P=3, norm=True, **xo)])])
    c["P2 res ln xout relu256 r15 N512"] = (15, [(512, True, 256, None, [dict(P=2, res=True, norm=True, **xo)])])
    c["three prologues r37"] = (37, [(256, True, None, None, [plain]), (256, False, None, None, [dict(res=True, norm=True)]),
                                     (256, False, None, None, [dict(res=True, norm=True)])])
    c["two branches r17"] = (17, [(256, True, None, None, [dict(norm=True, relu=True)]), (256, True, 0, None, [plain])])
    for rows in (37, 81):                # 3 x 35 x 3 = 315 workgroups: EARLY; 6 x 35 x 3 = 630: occupancy first
        c[f"10 256 2189 r{rows}"] = (rows, [(10, True, None, None, [dict(norm=True, relu=True)]), (256, True, 0, None, [plain]),
                                            (2189, False, None, (2192, 0), [dict(res=True, norm=True, **xo)])])
    for i, P in enumerate((2, 3, 4, 5, 16)):
        segs = [dict(P=P, scale=(0.25, -1.5)[i % 2], bias0=True, res=i % 2 == 0, norm=i != 3, **xo)] + [plain] * (i % 3)
        c[f"P{P} scale bias0 r{(1, 15, 16, 17, 37)[i]}"] = ((1, 15, 16, 17, 37)[i], [((10, 63, 64, 65, 512)[i], True, None, None, segs)])
    c["column slices r37 N2189"] = (37, [(2189, True, 1000, (2192, 0), [dict(ld=512, res=True, norm=True, x_ld=512, **xo), dict(ld=512)])])
    c["column slices r17 N65"] = (17, [(65, True, None, (512, 128), [dict(ld=2192, post=True, x_ld=2192, **xo)])])
    c["statistics r37 N64"] = (37, [(64, True, None, None, [dict(norm=True, **xo)])], tuple((17 + 2 * i, k) for i, k in enumerate(STATS)))
    c["statistics P3 res r37 N65"] = (37, [(65, True, None, None, [dict(P=3, res=True, norm=True, **xo), plain])],
                                      tuple((1 + 3 * i, k) for i, k in enumerate(STATS)))
    # (the NaN row with and without a ReLU behind it: rac_relu keeps a NaN as torch.relu does)
    c["nan row r37 N65"] = (37, [(65, True, None, None, [dict(res=True, norm=True, **xo)])], ((20, "nan"),))
    c["nan row relu r37 N65"] = (37, [(65, True, 0, None, [dict(norm=True, relu=True, **xo)])], ((21, "nan"),))
    return c


ROWGEMM_CASES = _rowgemm_cases()
ROWGEMM_INSTANTIATION = {"10 256 2189 r37": (1, 1, True), "10 256 2189 r81": (1, 1, False), "plain r16 2seg N1": (2, 1, True),
                         "plain r17 3seg N65": (3, 1, True), "column slices r37 N2189": (2, 1, True)}


def rowgemm_build(name):
    spec = ROWGEMM_CASES[name]
    rows, gemms, special = spec[0], spec[1], spec[2] if len(spec) > 2 else ()
    g = torch.Generator().manual_seed(2000 + list(ROWGEMM_CASES).index(name))
    out = []
    for N, bias, relu_from, out_ld, segs in gemms:
        out.append(gemm(g, [seg(g, rows, **kw) for kw in segs], N, bias, relu_from, out_ld))
    for row, kind in special:
        set_row(out[0]["segs"][0], row, kind)
    return dict(rows=rows, gemms=out, special=special)


def check_rowgemm(log, key, c, run):
    rows = c["rows"]
    launch, held = [], []
    for gm in c["gemms"]:
        full, region = guard(rows, gm["N"], *(gm["out_ld"] or (None, None)))
        full = run.dev(full)
        segs, dests = [], []
        for s in gm["segs"]:
            d = seg_on(run, s)
            xf = xr = im = ir = None
            if s["x_out"]:
                xf, xr = guard(rows, 256, *((s["x_ld"], s["x_ld"] - 260) if s["x_ld"] else (None, None)))
                xf = run.dev(xf)
            if s["split"]:
                im, ir = guard_image(rows, image_width(256, s["split"]))
                im = run.dev(im)
            d["x_out"], d["split_out"] = xf[xr] if xf is not None else None, im[ir] if im is not None else None
            segs.append(d)
            dests.append((xf, xr, im, ir))
        launch.append(dict(segs=segs, W=run.dev(gm["W"]), b=run.dev(gm["b"]) if gm["b"] is not None else None, out=full[region],
                           relu_from=gm["relu_from"], N=gm["N"]))
        held.append((full, region, dests))
    run.rowgemm(launch, rows)
    bounds = []
    for i, (gm, (full, region, dests)) in enumerate(zip(c["gemms"], held)):
        for j, (s, (xf, xr, im, ir)) in enumerate(zip(gm["segs"], dests)):
            if xf is not None:
                image = taken(run.host(im), ir) if im is not None else None
                check_finished_rows(log, f"rowgemm | {key} | gemm {i} x_out {j}", s, taken(run.host(xf), xr), image, c["special"] if i + j == 0 else ())
        out = taken(run.host(full), region)
        bounds.append(log.compare(f"rowgemm | {key} | gemm {i} out", out, gemm_value(gm, F64), gemm_mag(gm), gemm_value(gm, F32)))
        for row, kind in c["special"]:
            if kind == "nan" and i == 0:
                assert bool(torch.isnan(out[row]).all()) and not bool(torch.isnan(out[row - row % 16:row]).any())
    return bounds


# --------------------------------------------------------------------------------------------------------------- pe_head
def pe_case(seed, rows, zero_weight=False, nan_row=None):
    g = torch.Generator().manual_seed(seed)
    boxes = torch.rand(1, rows, 10, generator=g)
    if rows > 2:
        boxes[0, 1, :3] = 0                        # a row whose Linear output is the bias alone
    if nan_row is not None:
        boxes[0, nan_row, 1] = NAN
    W = torch.zeros(256, 3) if zero_weight else torch.randn(256, 3, generator=g)
    b = torch.full((256,), 0.75) if zero_weight else torch.randn(256, generator=g)
    return dict(boxes=boxes, W=W, b=b, gamma=torch.randn(256, generator=g), beta=torch.randn(256, generator=g), eps=LN_EPS,
                zero_weight=zero_weight, nan_row=nan_row)


def pe_value(x3, c, dtype, fault=None):
    v = x3.to(dtype) @ c["W"].to(dtype).t() + c["b"].to(dtype)
    return relu(layer_norm(v, c["gamma"], c["beta"], c["eps"]), fault)


def pe_mag(x3, c):
    """the LayerNorm rule with X_i = sum_j |W_ij| |x_j| + |b_i| (``x3`` in float64)"""
    X = x3.double().abs() @ c["W"].double().abs().t() + c["b"].double().abs()
    pre = x3.double() @ c["W"].double().t() + c["b"].double()
    return ln_magnitude(X, pre, c["gamma"], c["beta"], c["eps"])


def check_pe_head(log, key, c, run):
    boxes = run.dev(c["boxes"])
    x3 = c["boxes"][..., :3]
    out = run.host(run.pe_head(boxes[..., :3], *(run.dev(c[k]) for k in ("W", "b", "gamma", "beta")), c["eps"]))
    assert tuple(out.shape) == tuple(x3.shape[:-1]) + (256,)
    if c["zero_weight"]:                           # a constant Linear output: exactly relu(beta)
        assert torch.equal(out, torch.relu(c["beta"]).expand_as(out))
    bound = log.compare(f"pe_head | {key} | out", out, pe_value(x3, c, F64), pe_mag(x3, c), pe_value(x3, c, F32))
    if c["nan_row"] is not None:
        assert bool(torch.isnan(out[0, c["nan_row"]]).all()) and int(torch.isnan(out).any(-1).sum()) == 1
    return bound


# ------------------------------------------------------------------------------------------------ refine / layer boundary
EDGE = (0.0, 1.0, 1e-5, 1.0 - 1e-5, 5e-6, -0.1, 1.1)
POISON = ([NAN, math.inf, -math.inf, NAN, math.inf, -math.inf, 1.0, NAN, math.inf, -math.inf],
          [math.inf, NAN, 30.0, 0.0, 0.0, 0.0, NAN, 0.5, -math.inf, NAN])


def _templates():
    t = [dict(p={1: v, 2: EDGE[(i + 3) % 7]}) for i, v in enumerate(EDGE)]                  # inverse_sigmoid's clamps, d and z
    t += [dict(d={0: 30.0, 1: 30.0, 2: 30.0}), dict(d={0: -30.0, 1: -30.0, 2: -30.0}), dict(p={1: 0.0, 2: 1.0}, d={1: 30.0, 2: -30.0})]
    t += [dict(p={0: -0.3}), dict(p={0: 1.4})]                                              # theta leaving [0, 1]
    t += [dict(p={0: turn, 1: 0.97}, d={0: 0.0, 1: 3.0}) for turn in (0.0, 0.25, 0.5, 0.75)]   # x at 1, y at 1, x at 0, y at 0
    t += [dict(d={6: 0.0, 7: 0.0}), dict(d={3: 5.0, 4: -5.0, 5: 5.0}), dict(d={3: -5.0, 4: 5.0, 5: -5.0})]
    return t


TEMPLATES = _templates()
REFINE_SHAPES = {"BQ1": (1, 1), "BQ3": (1, 3), "BQ4": (1, 4), "BQ5": (1, 5), "B2 Q37": (2, 37)}


def refine_case(seed, B, Q, T, poison=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)                                            # noqa: E731
    prop = torch.cat([r(B, Q, 1), 0.05 + 0.9 * r(B, Q, 2), r(B, Q, 7) * 2 - 1], -1)
    delta = torch.randn(B, Q, 10, generator=g) * 0.7
    fp, fd = prop.view(-1, 10), delta.view(-1, 10)
    for i in range(B * Q):
        if B * Q > 5 and i % 2:                    # (ordinary rows between the edge rows where there is room)
            continue
        t = TEMPLATES[(i // (2 if B * Q > 5 else 1) + seed) % len(TEMPLATES)]
        for k, v in t.get("p", {}).items():
            fp[i, k] = v
        for k, v in t.get("d", {}).items():
            fd[i, k] = v
    td = torch.ones(B, T)
    if T > 1:
        td[:, 1:] = 0.3 + r(B, T - 1)
        td[:, 1] = torch.tensor([0.5, 1.5])[:B]    # the two batches differ
    rows = []
    if poison:
        rows = [1, B * Q - 2] if B * Q > 3 else [0]
        for row, vals in zip(rows, POISON):
            fd[row] = torch.tensor(vals)
    g2 = torch.Generator().manual_seed(seed + 1)
    pe = dict(W=torch.randn(256, 3, generator=g2), b=torch.randn(256, generator=g2), gamma=torch.randn(256, generator=g2),
              beta=torch.randn(256, generator=g2), eps=LN_EPS)
    return dict(B=B, Q=Q, T=T, prop=prop, delta=delta, td=td, poisoned=rows, pe=pe)


def refine_forward(c, dtype, fault=None):
    """-> (pred, xy, table) in ``dtype``: R.refine_bbox, the velocity / time_diff, R.theta_d2xy, R.decode_bbox"""
    p, d, td = (c[k].to(dtype) for k in ("prop", "delta", "td"))
    if fault == "other_batch_time_diff":
        td = td.flip(0)
    if fault == "no_eps_clamps":
        x = p[..., 1:3].clamp(min=0, max=1)
        dz = torch.sigmoid(d[..., 1:3] + torch.log(x / (1 - x)))
        pred = torch.cat([p[..., 0:1] + (torch.sigmoid(d[..., 0:1]) * 2 - 1) / NUM_RAY, dz, d[..., 3:]], -1)
    else:
        pred = R.refine_bbox(p, d, NUM_RAY)
    if c["T"] > 1:
        pred = torch.cat([pred[..., :8], pred[..., 8:] / td[:, 1:2, None]], -1)
    xy = R.theta_d2xy(pred)
    dec = R.decode_bbox(xy, PC)
    table = torch.cat([dec[..., :6], torch.cos(dec[..., 6:7]), torch.sin(dec[..., 6:7])], -1)
    return pred, xy, table


def _tame(t, nan_to=None):
    """+-inf -> +-FLT_MAX (what nan_to_num makes of them); NaN kept, or -> ``nan_to``"""
    t = t.double()
    return torch.nan_to_num(t, nan=NAN if nan_to is None else nan_to, posinf=FLT_MAX, neginf=-FLT_MAX)


def check_refine(log, key, c, run, boundary, fault_free=None):
    """rac_refine_fwd (boundary=False) or rac_layer_boundary_fwd against float64, column by column"""
    name = "layer_boundary" if boundary else "refine"
    B, Q = c["B"], c["Q"]
    restated = fault_free or Restated32()
    prop, delta, td = (run.dev(c[k]) for k in ("prop", "delta", "td"))
    p64, x64, t64 = refine_forward(c, F64)
    p32, x32, t32 = refine_forward(c, F32)
    if boundary:
        slots = run.dev(torch.full((3, B, Q, 10), NAN))
        res = run.layer_boundary(prop, delta, td, *(run.dev(c["pe"][k]) for k in ("W", "b", "gamma", "beta")), c["pe"]["eps"], slots[1])
        pred, xy, table, pe = (run.host(x) for x in res)
        slots = run.host(slots)
        assert bits_equal(slots[1], xy) and bool(torch.isnan(slots[0]).all()) and bool(torch.isnan(slots[2]).all())
    else:
        pred, xy = (run.host(x) for x in run.refine(prop, delta, td))
    # copies: columns 3-7 of pred and xy are the regression output itself, columns 8-9 of xy the velocities pred holds
    assert bits_equal(pred[..., 3:8], c["delta"][..., 3:8]) and bits_equal(xy[..., 3:8], c["delta"][..., 3:8])
    assert bits_equal(xy[..., 8:], pred[..., 8:])
    cols = [0, 1, 2, 8, 9]
    S = torch.ones(B, Q, 5, dtype=F64)
    S[..., 3:] = _tame(p64[..., 8:]).abs()
    log.compare(f"{name} | {key} | pred", _tame(pred[..., cols]), _tame(p64[..., cols]), S.nan_to_num(1.0), _tame(p32[..., cols]))
    # (the head applies nan_to_num to xy: the kernel's clamp already turns a NaN centre into 0)
    log.compare(f"{name} | {key} | xy", _tame(xy[..., :3], 0.0), _tame(x64[..., :3], 0.0), torch.ones(B, Q, 3, dtype=F64), _tame(x32[..., :3], 0.0))
    if not boundary:
        return
    keep = [i for i in range(B * Q) if i not in c["poisoned"]]
    flat = lambda x: x.reshape(B * Q, -1)[keep]                                            # noqa: E731
    St = torch.ones(B, Q, 8, dtype=F64)
    St[..., 0:3] = torch.tensor([max(abs(PC[i]), abs(PC[i + 3])) for i in range(3)], dtype=F64)
    St[..., 3:6] = t64[..., 3:6].abs() * (1 + p64[..., 3:6].abs())
    log.compare(f"{name} | {key} | table", flat(table), flat(t64), flat(St), flat(t32))
    x3 = p64[..., :3]
    # (every row: the position encoder's row of a poisoned box is NaN where float64's is, behind the ReLU too)
    log.compare(f"{name} | {key} | pe", pe, pe_value(x3, c["pe"], F64), pe_mag(x3, c["pe"]), pe_value(p32[..., :3], c["pe"], F32))
    if c["poisoned"]:
        assert bool(torch.isfinite(flat(table)).all()) and bool(torch.isfinite(flat(pe)).all())
        assert all(bool(torch.isnan(pe.reshape(B * Q, -1)[i]).all()) for i in c["poisoned"])
    # the fused launch against the separate ones: reported, not asserted
    pred2, xy2 = (run.host(x) for x in run.refine(prop, delta, td))
    table2 = run.host(run.box_prep(run.dev(pred2)))
    pe2 = run.host(run.pe_head(run.dev(pred2)[..., :3], *(run.dev(c["pe"][k]) for k in ("W", "b", "gamma", "beta")), c["pe"]["eps"]))
    same = dict(pred=bits_equal(pred, pred2), xy=bits_equal(xy, xy2), table=bits_equal(flat(table), flat(table2)), pe=bits_equal(flat(pe), flat(pe2)))
    print(f"{name} | {key}: bit-equal to refine_fused -> box_prep / pe_head: {same}")


# ---------------------------------------------------------------------------------------------------- gru_gate / upsample2x
def grid_stride(kernel, items):
    """whether a launch's threads take more than one item each: the launchers' workgroup caps"""
    cap = {"gru_gate": 4096, "upsample2x": 8192}[kernel]
    return items > min((items + 255) // 256, cap) * 256


GRU_CASES = {"chw4 B1": (1, 1, 2, 2, False), "chw4 B2 bias": (2, 1, 1, 4, True), "C6 5x7 B2 bias": (2, 6, 5, 8, True),
             "C6 5x7 B1": (1, 6, 5, 8, False), "C32 20x12 B2": (2, 32, 20, 12, False), "past the cap": (2, 64, 128, 260, True)}


def gru_case(name):
    B, C, H, W, bias = GRU_CASES[name]
    g = torch.Generator().manual_seed(3000 + list(GRU_CASES).index(name))
    gates = torch.randn(B, 3 * C, H, W, generator=g) * 2
    flat = gates.view(-1)
    flat[::7], flat[3::11] = 100.0, -100.0                                                 # saturated gates of both signs
    return dict(B=B, C=C, H=H, W=W, gates=gates, h_all=torch.randn(B, 3, C, H, W, generator=g),
                bias=torch.randn(3 * C, H, W, generator=g) if bias else None, items=B * C * H * W // 4)


def gru_value(c, dtype, fault=None):
    g = c["gates"].to(dtype)
    if c["bias"] is not None:
        g = g + c["bias"].to(dtype)
    h = c["h_all"][:, 1].to(dtype)
    zg, rg, cg = g.split(c["C"], dim=1)
    z, r = torch.sigmoid(zg), torch.sigmoid(rg)
    cand = torch.tanh(cg + r * h)
    return z * h + (1 - z) * cand if fault == "z_swapped" else (1 - z) * h + z * cand


def check_gru(log, key, c, run):
    B, C, H, W = c["B"], c["C"], c["H"], c["W"]
    h_all = run.dev(c["h_all"])
    out, out2 = run.dev(torch.full((B, 2, C, H, W), NAN)), run.dev(torch.full((B, 4, C, H, W), NAN))
    run.gru_gate(run.dev(c["gates"]), h_all[:, 1], out[:, 1], run.dev(c["bias"]) if c["bias"] is not None else None, out2[:, 2])
    out, out2 = run.host(out), run.host(out2)
    assert bool(torch.isnan(out[:, 0]).all()) and bool(torch.isnan(out2[:, [0, 1, 3]]).all()), "gru_gate wrote outside its [:, t] slots"
    assert bits_equal(out[:, 1], out2[:, 2])
    assert bits_equal(run.host(h_all), c["h_all"])
    return log.compare(f"gru_gate | {key} | h", out[:, 1], gru_value(c, F64), c["h_all"][:, 1].double().abs() + 1, gru_value(c, F32))


UPSAMPLE_CASES = {"1x2": (1, 1, 1, 2), "2x2 planes5": (1, 5, 2, 2), "3x4": (1, 1, 3, 4), "20x12 planes5": (5, 1, 20, 12),
                  "64x64": (1, 1, 64, 64), "past the cap": (2, 65, 128, 128)}


def upsample_case(name):
    N, C, h, w = UPSAMPLE_CASES[name]
    g = torch.Generator().manual_seed(4000 + list(UPSAMPLE_CASES).index(name))
    return dict(x=torch.randn(N, C, h, w, generator=g), items=N * C * 2 * h * (2 * w // 4))


def upsample64(x, magnitude=False, position=False):
    """bilinear x2 with align_corners: taps and weights in float64 from the integer ratio dst * (in - 1) / (out - 1).
    ``magnitude``: the same sum over |src|.  ``position``: what the tap positions contribute as inexact inputs, in units of 2^-24:
    kernel and torch form a position as float32(ratio) * index -- two float32 roundings, each at most 2^-24 of the position -- so
    the term is 2 * (pos_y * |d out / d pos_y| + pos_x * |d out / d pos_x|), the derivatives those of the bilinear sum itself."""
    x = x.double().abs() if magnitude else x.double()
    h, w = x.shape[-2:]

    def taps(n):
        pos = torch.arange(2 * n, dtype=F64) * (n - 1) / (2 * n - 1)
        i0 = pos.floor().long().clamp(max=n - 1)
        return i0, (i0 + 1).clamp(max=n - 1), pos - i0, pos
    y0, y1, ly, py = taps(h)
    x0, x1, lx, px = taps(w)
    ly, py = ly[:, None], py[:, None]
    a, b, c, d = x[..., y0, :][..., x0], x[..., y0, :][..., x1], x[..., y1, :][..., x0], x[..., y1, :][..., x1]
    top, bot = a * (1 - lx) + b * lx, c * (1 - lx) + d * lx
    if position:
        return 2 * (py * (bot - top).abs() + px * ((1 - ly) * (b - a) + ly * (d - c)).abs())
    return top * (1 - ly) + bot * ly


def check_upsample(log, key, c, run):
    """two comparisons with the same float64 reference.  The issue's magnitude A, the bilinear sum over |src|, treats the tap
    position as exact: on a large map the float32 position is what errs, E_ref (torch's own float32 result) reaches hundreds and
    the allowance with it.  The second magnitude adds the position's two roundings as an input term: E_ref stays of order 1 at
    every size, and a tap or weight that is off by more than the position's own rounding shows."""
    out = run.host(run.upsample2x(run.dev(c["x"])))
    r32 = TF.interpolate(c["x"], scale_factor=2, mode="bilinear", align_corners=True)
    ref, A = upsample64(c["x"]), upsample64(c["x"], magnitude=True)
    log.compare(f"upsample2x | {key} | out", out, ref, A, r32)
    return log.compare(f"upsample2x | {key} | out, positions inexact", out, ref, A + upsample64(c["x"], position=True), r32)


# ------------------------------------------------------------------------------------------------ the float32 restatement
FAULTS = ("variance_over_dim_minus_1", "eps_dropped", "partial_dropped", "scale_after_bias", "k_block_dropped", "relu_from_off_by_one",
          "residual_next_row", "other_batch_time_diff", "no_eps_clamps", "align_corners_false", "z_swapped", "relu_drops_nan")


class Restated32:
    """the same functions in float32 on the CPU; ``fault``: one of FAULTS, the deliberately wrong variant of a negative control"""

    def __init__(self, fault=None):
        assert fault is None or fault in FAULTS
        self.fault = fault

    def dev(self, t):
        return t

    def host(self, t):
        return t

    def _finish(self, s, x, x_out, split_out):
        if x_out is not None:
            x_out.copy_(x)
        if split_out is not None:
            split_out.copy_(split_image(x if x_out is None else x_out, s["split"]))

    def add_ln(self, s, out=None, split_out=None):
        x = pro_value(s, F32, self.fault)
        out = torch.empty_like(x) if out is None else out
        self._finish(s, x, out, split_out)
        return out

    def rowgemm(self, gemms, rows):
        for gm in gemms:
            for s in gm["segs"]:
                self._finish(s, pro_value(s, F32, self.fault), s["x_out"], s["split_out"])
            gm["out"].copy_(gemm_value(gm, F32, self.fault))

    def pe_head(self, x3, W, b, gamma, beta, eps):
        return pe_value(x3, dict(W=W, b=b, gamma=gamma, beta=beta, eps=eps), F32, self.fault)

    def refine(self, prop, delta, td):
        return refine_forward(dict(prop=prop, delta=delta, td=td, T=td.shape[1]), F32, self.fault)[:2]

    def box_prep(self, boxes):
        dec = R.decode_bbox(R.theta_d2xy(boxes), PC)
        return torch.cat([dec[..., :6], torch.cos(dec[..., 6:7]), torch.sin(dec[..., 6:7])], -1)

    def layer_boundary(self, prop, delta, td, W, b, gamma, beta, eps, xy_out):
        pred, xy, table = refine_forward(dict(prop=prop, delta=delta, td=td, T=td.shape[1]), F32, self.fault)
        xy_out.copy_(xy)
        return pred, xy_out, table, self.pe_head(pred[..., :3], W, b, gamma, beta, eps)

    def gru_gate(self, gates, h_prev, h_out, bias_map, h_out2):
        c = dict(gates=gates, bias=bias_map, h_all=torch.stack([h_prev, h_prev], 1), C=h_prev.shape[1])
        h_out.copy_(gru_value(c, F32, self.fault))
        if h_out2 is not None:
            h_out2.copy_(h_out)

    def upsample2x(self, x):
        return TF.interpolate(x, scale_factor=2, mode="bilinear", align_corners=self.fault != "align_corners_false")
