// resnet_bwd.hip -- backward of one Bottleneck convolution of the image backbone (resnet.hip's rn_conv_kernel) for gfx950, BatchNorms
// folded by the caller (eval statistics: the forward under autograd IS the folded convolution):
//
//   rac_resnet_conv_dgrad   dx[n][ci][p] = M( sum_{co,ky,kx} W[co][ci][ky][kx] * g[n][co][q] [+ add[n][ci][p]] ),
//                           over the (q, ky, kx) with stride * q + (ky, kx) - pad == p; M zeroes where mask[n][ci][p] <= 0
//   rac_resnet_conv_wgrad   dW[co][ci][ky][kx] = sum_{n,q} g[n][co][q] * x[n][ci][stride * q + (ky, kx) - pad],  db[co] = sum_{n,q} g[n][co][q]
//   rac_resnet_relu_bwd     out = y > 0 ? a [+ b] : 0
//
// Data gradient.  rn_conv_kernel with the roles of Cin and Cout exchanged and the taps flipped: an implicit GEMM whose "weights" are the
// line image of W^T as [Cin][K], K = (flipped tap, co), and whose "activations" are g.  At stride 1 that is the forward itself.  At
// stride 2 output pixel p reads tap t' at n = p + t' - pad only where both coordinates of n are even and n / 2 lies inside g: the staging
// step selects a zero for every other tap behind a clamped address, as the forward does at the border.  The output size H x W is an
// argument (7 and 8 both map to 4) and is checked against the forward's formula.  g's scale is one power of two per image
// (rac_resnet_absmax_fwd of g), the arithmetic the forward's: x * 2^e = hi + lo (two f16), lo*hi + hi*lo + hi*hi per K step in
// v_mfma_f32_16x16x32_f16, fp32 accumulate.  Workgroup = 4 waves, tile = 64 pixels of one image x 64 MI channels of dx (MI by the
// forward's rule).  The epilogue adds `add` (the identity branch, an outside gradient) and applies the ReLU backward of the layer in
// front (mask = the convolution's own post-ReLU input): a masked element is +0 exactly.
//
// Weight gradient.  fpn_lateral_bwd.hip's scheme for any Cout, taps and stride: K = N * Ho * Wo in units of 32 output pixels of one
// image, cut into k_splits contiguous ranges, none empty; a workgroup owns one range, one tap and a tile of 128 co x 128 ci (64 x 64
// where Cout is no multiple of 128 or Cin is below it; with 64 x 64 everywhere the f8 training step measured 104 ms, with the wide
// tiles 66 ms: a workgroup re-reads its operand rows per tile of products), and writes
// its partial sums to the workspace [k_splits][taps][Cout][Cin] (+ [k_splits][Cout] for db, by the workgroups of tap 0 / ci tile 0);
// a second launch adds the ranges in ascending order and stores torch's [Cout][Cin][k][k].  A row of the A operand is 32 consecutive
// pixels of one channel of g, a column of B the 32 pixels of one channel of x that this tap reads for them (zero outside the map, from
// a clamped address).  One power-of-two scale per channel and K range, from a first walk over the range (it factors out of a sum over
// pixels; a per-pixel or per-image scale would not); the two exact factors are multiplied back one after the other in the epilogue.
// All four products lo*lo + lo*hi + hi*lo + hi*hi: a 1 x 1 map of one image is a sum of ONE product, where the dropped lo*lo term
// (2^-22 of the product) beside the two operand roundings (2^-23 each) and the fp32 roundings measured 8.7 units of 2^-24 over the
// 10^6 weights of a 512 -> 2048 convolution; with it the bound is the operands' 2^-22.
// LDS rows of 64 B hi and 64 B lo, 16-byte slot s of row r at s ^ (3 * ((r >> 3) & 1)).
// No atomics, nothing read back, every sum in one fixed order, launch geometry from the shapes alone; 64-bit index arithmetic.
#include "rac_common.h"

typedef _Float16 rb_h8 __attribute__((ext_vector_type(8)));
typedef float rb_f4 __attribute__((ext_vector_type(4)));

#define RB_PARTS 64       // partial maxima per image (rac_resnet_absmax_fwd)
#define RB_ROW 80         // bytes per LDS pixel row of the data gradient: 32 f16 + 16 bytes of padding

// ------------------------------------------------------------------------------------------------ data gradient
struct RbDgradArgs {
    const float *g;       // [N][Cout][Ho*Wo]
    const char *w;        // [Cin][steps][hi 32 | lo 32] f16, step = flipped tap * (Cout / 32) + chunk
    const float *add;     // [N][Cin][H*W] or null
    const float *mask;    // [N][Cin][H*W] or null
    const float *parts;   // [N][RB_PARTS]
    float *out;           // [N][Cin][H*W]
    float w_alpha;
    int H, W, Ho, Wo, Cin, Cout, ksize, stride, pad, cblocks;
};

template <int MI>
__global__ __launch_bounds__(256) void rn_dgrad_kernel(const RbDgradArgs a)
{
    constexpr int HALF = 64 * RB_ROW;
    __shared__ __attribute__((aligned(16))) char rb_lds[2 * HALF];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int cb = blockIdx.x % a.cblocks;
    const long pt = blockIdx.x / a.cblocks;              // pixel tile over all images
    const int HW = a.H * a.W, tiles = (HW + 63) / 64;
    const int n = (int)(pt / tiles), p0 = (int)(pt - (long)n * tiles) * 64;
    const int ci0 = cb * 64 * MI + wave * 16 * MI;
    const int chunks = a.Cout >> 5, steps = a.ksize * a.ksize * chunks;
    const size_t HWo = (size_t)a.Ho * a.Wo;

    unsigned mb = rac_absbits(a.parts[(size_t)n * RB_PARTS + lane]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        mb = max(mb, (unsigned)__shfl_xor((int)mb, off));
    const float sc = rac_act_scale(__uint_as_float(mb));
    const float unscale = a.w_alpha / sc;                // both powers of two: exact

    // staging role: pixel sp of the tile, channels 8 sg .. 8 sg + 7 of the step's 32
    const int sp = tid & 63, sg = tid >> 6;
    const bool live = p0 + sp < HW;
    const int pc = live ? p0 + sp : HW - 1;
    const int ph = pc / a.W, pw = pc - ph * a.W;
    const float *__restrict__ gin = a.g + ((size_t)n * a.Cout + 8 * sg) * HWo;
    const int sh = a.stride - 1;                         // stride 1 or 2: a shift and a parity mask
    float rx[8];
    bool rvalid = false;
    auto gload = [&](int s) {
        const int tap = s / chunks, c = s - tap * chunks;
        const int ky = tap / a.ksize, kx = tap - ky * a.ksize;
        const int nh = ph + ky - a.pad, nw = pw + kx - a.pad;
        const int qh = nh >> sh, qw = nw >> sh;
        rvalid = live && nh >= 0 && nw >= 0 && ((nh | nw) & sh) == 0 && qh < a.Ho && qw < a.Wo;
        const int qhc = min(max(qh, 0), a.Ho - 1), qwc = min(max(qw, 0), a.Wo - 1);
        const float *p = gin + (size_t)c * 32 * HWo + (size_t)qhc * a.Wo + qwc;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            rx[e] = p[(size_t)e * HWo];
    };
    auto lstore = [&]() {
        rb_h8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = rvalid ? rx[e] * sc : 0.f;
            hi[e] = (_Float16)v;
            lo[e] = (_Float16)(v - (float)hi[e]);
        }
        char *d = rb_lds + sp * RB_ROW + 16 * sg;
        *reinterpret_cast<rb_h8 *>(d) = hi;
        *reinterpret_cast<rb_h8 *>(d + HALF) = lo;
    };

    const char *__restrict__ wrow = a.w + ((size_t)(ci0 + li) * steps) * 128 + lk * 16;
    const size_t wtile = (size_t)16 * steps * 128;

    rb_f4 acc[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[i][j] = (rb_f4){0.f, 0.f, 0.f, 0.f};

    gload(0);
    for (int s = 0; s < steps; ++s) {
        rb_h8 wh[MI], wl[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            wh[i] = *reinterpret_cast<const rb_h8 *>(wrow + i * wtile + (size_t)s * 128);
            wl[i] = *reinterpret_cast<const rb_h8 *>(wrow + i * wtile + (size_t)s * 128 + 64);
        }
        lstore();
        __syncthreads();
        if (s + 1 < steps)
            gload(s + 1);
        const char *S = rb_lds;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const char *b = S + (16 * j + li) * RB_ROW + 16 * lk;
            const rb_h8 xh = *reinterpret_cast<const rb_h8 *>(b);
            const rb_h8 xl = *reinterpret_cast<const rb_h8 *>(b + HALF);
#pragma unroll
            for (int i = 0; i < MI; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[i], xh, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[i], xl, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < MI; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[i], xh, acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // epilogue: accumulator tile (i, j) holds channels ci0 + 16 i + 4 lk + r (r = register) of pixel p0 + 16 j + li
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + 16 * j + li;
        if (p >= HW)
            continue;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int ci = ci0 + 16 * i + 4 * lk + r;
                const size_t o = ((size_t)n * a.Cin + ci) * HW + p;
                float v = acc[i][j][r] * unscale;
                if (a.add)
                    v += a.add[o];
                if (a.mask)
                    v = a.mask[o] <= 0.f ? 0.f : v;
                a.out[o] = v;
            }
    }
}

static bool rb_sizes_match(int H, int W, int Ho, int Wo, int ksize, int stride)
{
    const int pad = ksize / 2;
    return Ho == (H + 2 * pad - ksize) / stride + 1 && Wo == (W + 2 * pad - ksize) / stride + 1;
}

extern "C" int rac_resnet_conv_dgrad(const rac_resnet_dgrad *d, void *stream)
{
    const char *what = "rac_resnet_conv_dgrad";
    RAC_CHECK_ARG(d, "%s: null pointer (descriptor)", what);
    RAC_CHECK_ARG(d->ksize == 1 || d->ksize == 3, "%s: ksize=%d (1 or 3)", what, d->ksize);
    RAC_CHECK_ARG(d->stride == 1 || d->stride == 2, "%s: stride=%d (1 or 2)", what, d->stride);
    RAC_CHECK_ARG(d->Cin >= 64 && d->Cin % 64 == 0 && d->Cin <= 2048, "%s: Cin=%d (a multiple of 64, at most 2048)", what, d->Cin);
    RAC_CHECK_ARG(d->Cout >= 32 && d->Cout % 32 == 0 && d->Cout <= 2048, "%s: Cout=%d (a multiple of 32, at most 2048)", what, d->Cout);
    RAC_CHECK_ARG(d->N >= 1 && d->H >= 1 && d->W >= 1 && (long)d->H * d->W < (1l << 30), "%s: N=%d H=%d W=%d must be positive", what,
                  d->N, d->H, d->W);
    RAC_CHECK_ARG(d->Ho >= 1 && d->Wo >= 1 && rb_sizes_match(d->H, d->W, d->Ho, d->Wo, d->ksize, d->stride),
                  "%s: H=%d W=%d does not map to Ho=%d Wo=%d (ksize %d, stride %d)", what, d->H, d->W, d->Ho, d->Wo, d->ksize, d->stride);
    RAC_CHECK_ARG(d->g && d->w_image && d->amax_parts && d->out, "%s: null pointer", what);
    RAC_CHECK_ARG((reinterpret_cast<uintptr_t>(d->w_image) & 15) == 0, "%s: w_image must be 16-byte aligned", what);
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(d->g) | reinterpret_cast<uintptr_t>(d->out) | reinterpret_cast<uintptr_t>(d->add) |
                    reinterpret_cast<uintptr_t>(d->mask) | reinterpret_cast<uintptr_t>(d->amax_parts)) & 3) == 0,
                  "%s: g / add / mask / amax_parts / out must be 4-byte aligned", what);
    RbDgradArgs a;
    a.g = d->g; a.w = reinterpret_cast<const char *>(d->w_image); a.add = d->add; a.mask = d->mask; a.parts = d->amax_parts;
    a.out = d->out; a.w_alpha = d->w_alpha;
    a.H = d->H; a.W = d->W; a.Ho = d->Ho; a.Wo = d->Wo; a.Cin = d->Cin; a.Cout = d->Cout; a.ksize = d->ksize; a.stride = d->stride;
    a.pad = d->ksize / 2;
    // the forward's tile rule on the channels of dx
    const long ptiles = (long)d->N * ((a.H * a.W + 63) / 64);
    int mi = 1;
    for (int c = 4; c > 1; c >>= 1)
        if (d->Cin % (64 * c) == 0 && ptiles * (d->Cin / (64 * c)) >= 256) {
            mi = c;
            break;
        }
    a.cblocks = d->Cin / (64 * mi);
    const long wgs = ptiles * a.cblocks;
    RAC_CHECK_ARG(wgs < (1l << 31), "%s: %ld workgroups", what, wgs);
    const dim3 grid((unsigned)wgs);
    hipStream_t st = (hipStream_t)stream;
    if (mi == 4) hipLaunchKernelGGL(rn_dgrad_kernel<4>, grid, dim3(256), 0, st, a);
    else if (mi == 2) hipLaunchKernelGGL(rn_dgrad_kernel<2>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(rn_dgrad_kernel<1>, grid, dim3(256), 0, st, a);
    return rac_launch_status(what);
}

// ------------------------------------------------------------------------------------------------ weight and bias gradients
struct RbWgradArgs {
    const float *g;      // [N][Cout][Ho*Wo]
    const float *x;      // [N][Cin][H*W]
    float *ws;           // [k_splits][taps][Cout][Cin] partial sums
    float *wsb;          // [k_splits][Cout] partial bias sums, or null
    int Cin, Cout, H, W, Ho, Wo, ksize, stride, pad, taps;
    int upi, units, per, cotiles, citiles;      // upi: units of 32 output pixels per image; per: units per K range
};

__device__ __forceinline__ int rb_slot(int row, int s) { return s ^ (3 * ((row >> 3) & 1)); }

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
        float m = mx[j];
        m = fmaxf(m, __shfl_xor(m, 1));
        m = fmaxf(m, __shfl_xor(m, 2));
        // 2^(13 - e) with e = floor(log2(max)), exponent arithmetic only (max = 0 / denormal / inf: clamped exponents)
        int eb = (int)((__float_as_uint(m) >> 23) & 255u);
        eb = eb < 14 ? 14 : (eb > 254 ? 254 : eb);
        sc[j] = __uint_as_float((unsigned)(267 - eb) << 23);
        if (s_q == 0)
            rb_unscale[64 * j + s_r] = __uint_as_float((unsigned)(eb - 13) << 23);
    }
    if (do_bias) {
#pragma unroll
        for (int j = 0; j < NPG; ++j) {
            float t = bs[j];
            t += __shfl_xor(t, 1);
            t += __shfl_xor(t, 2);
            if (s_q == 0)
                a.wsb[(size_t)split * a.Cout + COT * cot + 64 * j + s_r] = t;
        }
    }

    // ---- second walk: the products.  Wave w owns co 16 NI w .. 16 NI (w + 1) - 1 of the tile x its CIT ci = NI x NJ MFMA tiles.
    rb_f4 acc[NI][NJ];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            acc[i][j] = (rb_f4){0.f, 0.f, 0.f, 0.f};
    const int a_off = (16 * NI * wave + li) * 64 + 16 * rb_slot(li, lk);      // tile i: + 1024 i  (row & 8 == li & 8)
    const int b_off = (COT + li) * 64 + 16 * rb_slot(li, lk);                // tile j: + 1024 j
    float rx[NP][8];
    gload(u0, rx);
    for (int u = u0; u < u1; ++u) {
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const int row = 64 * j + s_r;
            rb_h8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float s = rx[j][e] * sc[j];
                hi[e] = (_Float16)s;
                lo[e] = (_Float16)(s - (float)hi[e]);
            }
            char *d = rb_lds + row * 64 + 16 * rb_slot(row, s_q);
            *reinterpret_cast<rb_h8 *>(d) = hi;
            *reinterpret_cast<rb_h8 *>(d + HALF) = lo;
        }
        __syncthreads();
        if (u + 1 < u1)
            gload(u + 1, rx);
        rb_h8 ah[NI], al[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            ah[i] = *reinterpret_cast<const rb_h8 *>(rb_lds + a_off + 1024 * i);
            al[i] = *reinterpret_cast<const rb_h8 *>(rb_lds + HALF + a_off + 1024 * i);
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const rb_h8 bh = *reinterpret_cast<const rb_h8 *>(rb_lds + b_off + 1024 * j);
            const rb_h8 bl = *reinterpret_cast<const rb_h8 *>(rb_lds + HALF + b_off + 1024 * j);
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bl, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh, acc[i][j], 0, 0, 0);
            }
        }
        __syncthreads();      // every wave has read the stage: the next unit may overwrite it
    }

    // ---- epilogue.  Accumulator tile (i, j): rows 4 lk + r = co, column li = ci.  (Two exact power-of-two factors one after the
    // other: their product could leave the float range.)
    float *__restrict__ wp = a.ws + ((size_t)split * a.taps + tap) * a.Cout * a.Cin;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int ci = CIT * cit + 16 * j + li;
        if (ci < a.Cin) {
            const float ux = rb_unscale[COT + 16 * j + li];
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int col = 16 * (NI * wave + i) + 4 * lk + r;
                    wp[(size_t)(COT * cot + col) * a.Cin + ci] = acc[i][j][r] * rb_unscale[col] * ux;
                }
        }
    }
}

// dW[co][ci][tap] = the k_splits partial sums added in ascending order; db likewise
__global__ __launch_bounds__(256) void rn_wgrad_reduce_kernel(const float *__restrict__ ws, const float *__restrict__ wsb,
                                                              float *__restrict__ dw, float *__restrict__ db, int Cout, int Cin,
                                                              int taps, int k_splits)
{
    const long total = (long)Cout * Cin * taps;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < total) {
        const int tap = (int)(e % taps);
        const long r = e / taps;
        const int ci = (int)(r % Cin), co = (int)(r / Cin);
        const size_t at = ((size_t)tap * Cout + co) * Cin + ci;
        float s = 0.f;
        for (int p = 0; p < k_splits; ++p)
            s += ws[(size_t)p * total + at];
        dw[e] = s;
    } else if (db && e < total + Cout) {
        const int co = (int)(e - total);
        float s = 0.f;
        for (int p = 0; p < k_splits; ++p)
            s += wsb[(size_t)p * Cout + co];
        db[co] = s;
    }
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
    RAC_CHECK_ARG(Ho >= 1 && Wo >= 1 && rb_sizes_match(H, W, Ho, Wo, ksize, stride),
                  "%s: H=%d W=%d does not map to Ho=%d Wo=%d (ksize %d, stride %d)", what, H, W, Ho, Wo, ksize, stride);
    const int HWo = Ho * Wo, upi = (HWo + 31) / 32;
    RAC_CHECK_ARG((long)N * upi < (1l << 31), "%s: N=%d Ho=%d Wo=%d (too many K units)", what, N, Ho, Wo);
    const int units = N * upi;
    RAC_CHECK_ARG(k_splits >= 1 && k_splits <= units, "%s: k_splits=%d (1 .. %d units of 32 pixels)", what, k_splits, units);
    const int per = (units + k_splits - 1) / k_splits;
    RAC_CHECK_ARG((long)(k_splits - 1) * per < units, "%s: k_splits=%d leaves an empty range (%d units, %d per range)", what, k_splits,
                  units, per);
    RAC_CHECK_ARG(g && x && workspace && dw, "%s: null pointer", what);
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(workspace) |
                    reinterpret_cast<uintptr_t>(dw) | reinterpret_cast<uintptr_t>(db)) & 3) == 0,
                  "%s: pointers must be 4-byte aligned", what);
    RbWgradArgs a;
    a.g = g; a.x = x; a.ws = workspace;
    a.taps = ksize * ksize;
    a.wsb = db ? workspace + (size_t)k_splits * a.taps * Cout * Cin : nullptr;
    a.Cin = Cin; a.Cout = Cout; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.ksize = ksize; a.stride = stride; a.pad = ksize / 2;
    // tiles of 128 co x 128 ci (a quarter of the operand traffic per product) where Cout has them and Cin fills one, 64 x 64 below
    const bool wide = Cout % 128 == 0 && Cin >= 128;
    const int tile = wide ? 128 : 64;
    a.upi = upi; a.units = units; a.per = per; a.cotiles = Cout / tile; a.citiles = (Cin + tile - 1) / tile;
    const long wgs = (long)k_splits * a.taps * a.cotiles * a.citiles;
    RAC_CHECK_ARG(wgs < (1l << 31), "%s: %ld workgroups", what, wgs);
    hipStream_t st = (hipStream_t)stream;
    if (wide) hipLaunchKernelGGL((rn_wgrad_kernel<2, 8>), dim3((unsigned)wgs), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((rn_wgrad_kernel<1, 4>), dim3((unsigned)wgs), dim3(256), 0, st, a);
    const long outs = (long)Cout * Cin * a.taps + Cout;
    hipLaunchKernelGGL(rn_wgrad_reduce_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, workspace, a.wsb, dw, db, Cout,
                       Cin, a.taps, k_splits);
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
