// resnet_bwd.hip -- backward of one Bottleneck convolution of the image backbone (resnet.hip's rn_conv_kernel) for gfx950, BatchNorms
// folded by the caller (eval statistics: the forward under autograd IS the folded convolution):
//
//   rac_resnet_conv_wgrad   dW[co][ci][ky][kx] = sum_{n,q} g[n][co][q] * x[n][ci][stride * q + (ky, kx) - pad],  db[co] = sum_{n,q} g[n][co][q]
//   rac_resnet_relu_bwd     out = y > 0 ? a [+ b] : 0
//
// The data gradient (rac_resnet_conv_dgrad) is the forward's kernel under its second rule, in resnet.hip.
//
// Weight gradient.  The split-K scheme of wgrad_splitk.h (shared with fpn_lateral_bwd.hip) for any Cout, taps and stride: K = N * Ho * Wo
// in units of 32 output pixels of one image; a workgroup owns one K range, one tap and a tile of 128 co x 128 ci (64 x 64
// where Cout is no multiple of 128 or Cin is below it; with 64 x 64 everywhere the f8 training step measured 104 ms, with the wide
// tiles 66 ms: a workgroup re-reads its operand rows per tile of products), and writes
// its partial sums to the workspace [k_splits][taps][Cout][Cin] (+ [k_splits][Cout] for db, by the workgroups of tap 0 / ci tile 0);
// the reduce launch stores torch's [Cout][Cin][k][k].  A row of the A operand is 32 consecutive
// pixels of one channel of g, a column of B the 32 pixels of one channel of x that this tap reads for them (zero outside the map, from
// a clamped address; a per-pixel or per-image scale would not factor out of the sum over pixels, the per-channel one does).
// All four products lo*lo + lo*hi + hi*lo + hi*hi: a 1 x 1 map of one image is a sum of ONE product, where the dropped lo*lo term
// (2^-22 of the product) beside the two operand roundings (2^-23 each) and the fp32 roundings measured 8.7 units of 2^-24 over the
// 10^6 weights of a 512 -> 2048 convolution; with it the bound is the operands' 2^-22.
// No atomics, nothing read back, every sum in one fixed order, launch geometry from the shapes alone; 64-bit index arithmetic.
#include "wgrad_splitk.h"

// ------------------------------------------------------------------------------------------------ weight and bias gradients
struct RbWgradArgs {
    const float *g;      // [N][Cout][Ho*Wo]
    const float *x;      // [N][Cin][H*W]
    float *ws;           // [k_splits][taps][Cout][Cin] partial sums
    float *wsb;          // [k_splits][Cout] partial bias sums, or null
    int Cin, Cout, H, W, Ho, Wo, ksize, stride, pad, taps;
    int upi, units, per, cotiles, citiles;      // upi: units of 32 output pixels per image; per: units per K range
};

// NI: 16-channel MFMA tiles of co per wave (1: 64 co per workgroup, 2: 128); NJ: 16-channel tiles of ci per workgroup (4: 64, 8: 128)
template <int NI, int NJ>
__global__ __launch_bounds__(256, 2) void rn_wgrad_kernel(const RbWgradArgs a)
{
    constexpr int COT = 64 * NI, CIT = 16 * NJ;
    constexpr int ROWS = COT + CIT;         // LDS rows: the tile's channels of g, then its channels of x
    constexpr int NPG = COT / 64, NP = ROWS / 64;      // staging passes of 64 rows: g's, then x's
    constexpr int HALF = ROWS * 64;         // bytes of the hi image (the lo image follows)
    __shared__ __attribute__((aligned(16))) char rb_lds[2 * HALF];
    __shared__ float rb_unscale[ROWS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    long b = blockIdx.x;
    const int cit = (int)(b % a.citiles);
    b /= a.citiles;
    const int cot = (int)(b % a.cotiles);
    b /= a.cotiles;
    const int tap = (int)(b % a.taps), split = (int)(b / a.taps);
    const int ky = tap / a.ksize, kx = tap - ky * a.ksize;
    const int u0 = split * a.per, u1 = min(u0 + a.per, a.units);
    const int HWo = a.Ho * a.Wo;
    const size_t HWi = (size_t)a.H * a.W;

    // staging role: pass j = row 64 j + s_r of the block, pixels 8 s_q .. 8 s_q + 7 of the unit
    const int s_r = tid >> 2, s_q = tid & 3;
    size_t rowoff[NP];                      // the row's channel offset inside one image of g (j < NPG) or of x
#pragma unroll
    for (int j = 0; j < NP; ++j)
        rowoff[j] = j < NPG ? (size_t)(COT * cot + 64 * j + s_r) * HWo
                            : (size_t)min(CIT * cit + 64 * (j - NPG) + s_r, a.Cin - 1) * HWi;
    auto gload = [&](int u, float (&r)[NP][8]) {
        const int n = u / a.upi, q0 = (u - n * a.upi) * 32 + 8 * s_q;
        const float *__restrict__ gn = a.g + (size_t)n * a.Cout * HWo;
        const float *__restrict__ xn = a.x + (size_t)n * a.Cin * HWi;
        // the 8 pixels' addresses in g and, through this tap, in x: one division, then a walk along the row
        int goff[8], xoff[8];
        unsigned lm = 0u, vm = 0u;
        const int q0c = min(q0, HWo - 1);
        int oh = q0c / a.Wo, ow = q0c - oh * a.Wo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const bool live = q0 + e < HWo;
            goff[e] = min(q0 + e, HWo - 1);
            const int ih = oh * a.stride + ky - a.pad, iw = ow * a.stride + kx - a.pad;
            const bool valid = live && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
            xoff[e] = min(max(ih, 0), a.H - 1) * a.W + min(max(iw, 0), a.W - 1);
            lm |= (unsigned)live << e;
            vm |= (unsigned)valid << e;
            if (++ow == a.Wo) {
                ow = 0;
                ++oh;
            }
        }
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = j < NPG ? gn[rowoff[j] + goff[e]] : xn[rowoff[j] + xoff[e]];
                r[j][e] = ((j < NPG ? lm : vm) >> e) & 1u ? v : 0.f;
            }
    };

    // ---- first walk: per-channel maxima over this K range (and the bias sums, by the workgroups of tap 0 and ci tile 0)
    const bool do_bias = a.wsb != nullptr && tap == 0 && cit == 0;
    float mx[NP], bs[NPG];
#pragma unroll
    for (int j = 0; j < NP; ++j)
        mx[j] = 0.f;
#pragma unroll
    for (int j = 0; j < NPG; ++j)
        bs[j] = 0.f;
    for (int u = u0; u < u1; ++u) {
        float r[NP][8];
        gload(u, r);
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e)
                mx[j] = fmaxf(mx[j], fabsf(r[j][e]));
        if (do_bias) {
#pragma unroll
            for (int j = 0; j < NPG; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    bs[j] += r[j][e];
        }
    }
    float sc[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        float us;
        sc[j] = wg_row_scale(mx[j], us);
        if (s_q == 0)
            rb_unscale[64 * j + s_r] = us;
    }
    if (do_bias) {
#pragma unroll
        for (int j = 0; j < NPG; ++j) {
            const float t = wg_row_sum(bs[j]);
            if (s_q == 0)
                a.wsb[(size_t)split * a.Cout + COT * cot + 64 * j + s_r] = t;
        }
    }

    // ---- second walk: the products.  Wave w owns co 16 NI w .. 16 NI (w + 1) - 1 of the tile x its CIT ci = NI x NJ MFMA tiles.
    rac_f4v acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            acc[i][j] = (rac_f4v){0.f, 0.f, 0.f, 0.f};
    const int a_off = wg_frag_off(16 * NI * wave, li, lk), b_off = wg_frag_off(COT, li, lk);
    float rx[NP][8];
    gload(u0, rx);
    for (int u = u0; u < u1; ++u) {
#pragma unroll
        for (int j = 0; j < NP; ++j)
            wg_stage(rb_lds, HALF, 64 * j + s_r, s_q, sc[j], [&](int e) { return rx[j][e]; });
        __syncthreads();
        if (u + 1 < u1)
            gload(u + 1, rx);
        wg_products<4>(rb_lds, HALF, a_off, b_off, acc);
        __syncthreads();      // every wave has read the stage: the next unit may overwrite it
    }

    float *wp = a.ws + (((size_t)split * a.taps + tap) * a.Cout + COT * cot) * a.Cin;
    wg_store(wp, rb_unscale, COT, acc, CIT * cit, a.Cin, wave, li, lk);
}

extern "C" int rac_resnet_conv_wgrad(const float *g, const float *x, float *workspace, float *dw, float *db, int N, int Cin, int H,
                                     int W, int Cout, int Ho, int Wo, int ksize, int stride, int k_splits, void *stream)
{
    const char *what = "rac_resnet_conv_wgrad";
    RAC_CHECK_ARG(ksize == 1 || ksize == 3, "%s: ksize=%d (1 or 3)", what, ksize);
    RAC_CHECK_ARG(stride == 1 || stride == 2, "%s: stride=%d (1 or 2)", what, stride);
    RAC_CHECK_ARG(Cin >= 32 && Cin % 32 == 0 && Cin <= 2048, "%s: Cin=%d (a multiple of 32, at most 2048)", what, Cin);
    RAC_CHECK_ARG(Cout >= 64 && Cout % 64 == 0 && Cout <= 2048, "%s: Cout=%d (a multiple of 64, at most 2048)", what, Cout);
    RAC_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && (long)H * W < (1l << 30), "%s: N=%d H=%d W=%d must be positive", what, N, H, W);
    RAC_CHECK_ARG(Ho >= 1 && Wo >= 1 && Ho == rac_conv_out_size(H, ksize, stride) && Wo == rac_conv_out_size(W, ksize, stride),
                  "%s: H=%d W=%d does not map to Ho=%d Wo=%d (ksize %d, stride %d)", what, H, W, Ho, Wo, ksize, stride);
    WgSplit ks;
    if (const int rc = wg_split(what, "Ho", "Wo", N, Ho, Wo, k_splits, g, x, workspace, dw, db, ks))
        return rc;
    RbWgradArgs a;
    a.g = g; a.x = x; a.ws = workspace;
    a.taps = ksize * ksize;
    a.wsb = db ? workspace + (size_t)k_splits * a.taps * Cout * Cin : nullptr;
    a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.ksize = ksize; a.stride = stride; a.pad = ksize / 2;
    // tiles of 128 co x 128 ci (a quarter of the operand traffic per product) where Cout has them and Cin fills one, 64 x 64 below
    const bool wide = Cout % 128 == 0 && Cin >= 128;
    const int tile = wide ? 128 : 64;
    a.upi = ks.upi; a.units = ks.units; a.per = ks.per; a.cotiles = Cout / tile; a.citiles = (Cin + tile - 1) / tile;
    const long wgs = (long)k_splits * a.taps * a.cotiles * a.citiles;
    RAC_CHECK_ARG(wgs < (1l << 31), "%s: %ld workgroups", what, wgs);
    hipStream_t st = (hipStream_t)stream;
    if (wide) hipLaunchKernelGGL((rn_wgrad_kernel<2, 8>), dim3((unsigned)wgs), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((rn_wgrad_kernel<1, 4>), dim3((unsigned)wgs), dim3(256), 0, st, a);
    wg_reduce(workspace, a.wsb, dw, db, Cout, Cin, a.taps, k_splits, st);
    return rac_launch_status(what);
}

// ------------------------------------------------------------------------------------------------ ReLU backward
__global__ __launch_bounds__(256) void rn_relu_bwd_kernel(const float *__restrict__ y, const float *__restrict__ a,
                                                          const float *__restrict__ b, float *__restrict__ out, long count)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= count)
        return;
    const float v = b ? a[i] + b[i] : a[i];
    out[i] = y[i] > 0.f ? v : 0.f;
}

extern "C" int rac_resnet_relu_bwd(const float *y, const float *a, const float *b, float *out, int64_t count, void *stream)
{
    const char *what = "rac_resnet_relu_bwd";
    RAC_CHECK_ARG(count >= 1 && (count + 255) / 256 < (1l << 31), "%s: count=%ld", what, (long)count);
    RAC_CHECK_ARG(y && a && out, "%s: null pointer", what);
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) |
                    reinterpret_cast<uintptr_t>(out)) & 3) == 0,
                  "%s: pointers must be 4-byte aligned", what);
    hipLaunchKernelGGL(rn_relu_bwd_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y, a, b, out,
                       (long)count);
    return rac_launch_status(what);
}
