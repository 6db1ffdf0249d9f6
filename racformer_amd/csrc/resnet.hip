// resnet.hip -- the image backbone (mmdet ResNet, Bottleneck depths, style 'pytorch', eval-mode BatchNorms folded by the caller) for
// gfx950: the stem (7x7 / stride 2 convolution, ReLU, 3x3 / stride 2 max pool) and one convolution of a Bottleneck with its epilogue,
//
//   out[n][co][q] = [relu]( sum W[co][ci][ky][kx] * in[n][ci][s q + (ky, kx) - pad] + bias[co] [+ residual[n][co][q]] ),
//
// channel-first f32 in and out, so a stage's last block writes what the necks (fpn_lateral.hip) read.
//
// rn_conv_kernel: an implicit GEMM on the f16 matrix cores with the project's split-precision arithmetic (x * 2^e = hi + lo, two f16;
// weight image [Cout][K/32][hi 32 | lo 32] from rac_gemm_split_pack_fwd with K = (tap, ci), tap-major; the three leading products
// lo*hi + hi*lo + hi*hi per K step in v_mfma_f32_16x16x32_f16, fp32 accumulate).  The activation scale 2^e is chosen PER IMAGE: a 3x3
// sum reads a different pixel with every tap, so fpn_lateral.hip's per-pixel scale does not factor out of it; the image's maximum comes
// from a pass of its own (rn_absmax_kernel: RN_PARTS partial maxima per image, combined by every workgroup of the convolution -- a maximum
// has no order, nothing is atomic).  One scale rule for 1x1 and 3x3 keeps one kernel.
//
// Workgroup = 256 threads = 4 waves, tile = 64 consecutive output pixels of ONE image x 64 MI output channels (MI = 4, 2 or 1: the
// widest that divides Cout and still gives every CU a workgroup, 64 channels below -- a function of the shapes alone); a wave owns 16 MI channels x the 64 pixels = MI x 4 MFMA tiles.  K steps of 32
// input channels of one tap: thread (pixel sp, channel group sg) loads its pixel's 8 channels (consecutive lanes = consecutive pixels:
// coalesced along the row at stride 1), scales, splits and stores 16 bytes of hi and of lo to LDS rows [pixel][32 channels], which is
// what the MFMA's B operand reads back (lane (li, lk): pixel li, channels 8 lk .. 8 lk + 7: one 16-byte read).  Taps outside the map are
// zeros (the load re-reads a clamped address, the value is selected).  The weights are the A operand, read from their line image
// directly.  The activation loads of step s + 1 are in flight under the MFMAs of step s; one LDS stage, two barriers per step -- two stages
// with one barrier, with or without the weights one step ahead in registers, were measured slower (144 -> 172 registers
// at MI = 4 takes the third wave from each SIMD).
// Workgroups of one pixel tile are neighbours in the grid (channel block fastest), so the tile's input is shared through L2.
//
// rn_stem_kernel: exact fp32 (an fmaf chain over (ci, ky, kx) in ascending order per output).  K = 147 is no multiple of the MFMA's 32
// and the layer is bound by its 554 MB of output at the f8 shapes, not by arithmetic.  A workgroup owns 16 x 16 convolution outputs of
// one image x all 64 channels: weights [147][64] and the 37 x 37 x 3 input patch in LDS, the optional input normalisation
// (x[perm[c]] - mean[c]) / std[c] (IEEE division) applied while the patch is staged; padding stays zero.  rn_pool_kernel then takes the
// maximum of the valid pixels of each 3x3 / stride 2 / pad 1 window.
// No atomics, nothing read back, every sum in one fixed order, launch geometry from the shapes alone; 64-bit index arithmetic.
#include "rac_common.h"

typedef _Float16 rn_h8 __attribute__((ext_vector_type(8)));
typedef float rn_f4 __attribute__((ext_vector_type(4)));

#define RN_PARTS 64       // partial maxima per image (rac_resnet_absmax_fwd)
#define RN_ROW 80         // bytes per LDS pixel row: 32 f16 + 16 bytes of padding (spreads the 16-byte reads over the banks)
#define RN_STEM_C 64
#define RN_STEM_TAPS 147
#define RN_STEM_PATCH 37  // (16 - 1) * 2 + 7

// ------------------------------------------------------------------------------------------------ per-image maximum
__global__ __launch_bounds__(256) void rn_absmax_kernel(const float *__restrict__ x, float *__restrict__ parts, long per_image)
{
    __shared__ unsigned red[4];
    const int n = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const long len = (per_image + RN_PARTS - 1) / RN_PARTS;
    const long b = (long)part * len, e = b + len < per_image ? b + len : per_image;
    const float *__restrict__ xn = x + (size_t)n * per_image;
    unsigned m = 0u;
    for (long i = b + tid; i < e; i += 256)
        m = max(m, rac_absbits(xn[i]));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        m = max(m, (unsigned)__shfl_xor((int)m, off));
    if ((tid & 63) == 0)
        red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0)
        parts[(size_t)n * RN_PARTS + part] = __uint_as_float(max(max(red[0], red[1]), max(red[2], red[3])));
}

extern "C" int rac_resnet_absmax_fwd(const float *x, float *parts, int N, int64_t per_image, void *stream)
{
    const char *what = "rac_resnet_absmax_fwd";
    RAC_CHECK_ARG(N >= 1 && N <= 65535 && per_image >= 1, "%s: N=%d per_image=%ld", what, N, (long)per_image);
    RAC_CHECK_ARG(x && parts, "%s: null pointer", what);
    hipLaunchKernelGGL(rn_absmax_kernel, dim3(RN_PARTS, (unsigned)N), dim3(256), 0, (hipStream_t)stream, x, parts, (long)per_image);
    return rac_launch_status(what);
}

// ------------------------------------------------------------------------------------------------ Bottleneck convolution
struct RnConvArgs {
    const float *in;      // [N][Cin][H*W]
    const char *w;        // [Cout][steps][hi 32 | lo 32] f16, step = tap * (Cin / 32) + chunk
    const float *bias;    // [Cout] or null
    const float *res;     // [N][Cout][Ho*Wo] or null
    const float *parts;   // [N][RN_PARTS]
    float *out;           // [N][Cout][Ho*Wo]
    float w_alpha;
    int relu, H, W, Ho, Wo, Cin, Cout, ksize, stride, pad, cblocks;
};

template <int MI>
__global__ __launch_bounds__(256) void rn_conv_kernel(const RnConvArgs a)
{
    constexpr int HALF = 64 * RN_ROW;
    __shared__ __attribute__((aligned(16))) char rn_lds[2 * HALF];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int cb = blockIdx.x % a.cblocks;
    const long pt = blockIdx.x / a.cblocks;              // pixel tile over all images
    const int HWo = a.Ho * a.Wo, tiles = (HWo + 63) / 64;
    const int n = (int)(pt / tiles), q0 = (int)(pt - (long)n * tiles) * 64;
    const int co0 = cb * 64 * MI + wave * 16 * MI;
    const int chunks = a.Cin >> 5, steps = a.ksize * a.ksize * chunks;
    const size_t HWi = (size_t)a.H * a.W;

    // the image's scale: every wave combines the RN_PARTS partial maxima (bit patterns: a NaN wins and turns the scale into 1)
    unsigned mb = rac_absbits(a.parts[(size_t)n * RN_PARTS + lane]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        mb = max(mb, (unsigned)__shfl_xor((int)mb, off));
    const float sc = rac_act_scale(__uint_as_float(mb));
    const float unscale = a.w_alpha / sc;                // both powers of two: exact

    // staging role: pixel sp of the tile, channels 8 sg .. 8 sg + 7 of the step's 32
    const int sp = tid & 63, sg = tid >> 6;
    const bool live = q0 + sp < HWo;
    const int qc = live ? q0 + sp : HWo - 1;
    const int oh = qc / a.Wo, ow = qc - oh * a.Wo;
    const float *__restrict__ xin = a.in + ((size_t)n * a.Cin + 8 * sg) * HWi;
    float rx[8];
    bool rvalid = false;
    auto gload = [&](int s) {
        const int tap = s / chunks, c = s - tap * chunks;
        const int ky = tap / a.ksize, kx = tap - ky * a.ksize;
        const int ih = oh * a.stride + ky - a.pad, iw = ow * a.stride + kx - a.pad;
        rvalid = live && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W;
        const int ihc = min(max(ih, 0), a.H - 1), iwc = min(max(iw, 0), a.W - 1);
        const float *p = xin + (size_t)c * 32 * HWi + (size_t)ihc * a.W + iwc;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            rx[e] = p[(size_t)e * HWi];
    };
    auto lstore = [&]() {
        rn_h8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = rvalid ? rx[e] * sc : 0.f;
            hi[e] = (_Float16)v;
            lo[e] = (_Float16)(v - (float)hi[e]);
        }
        char *d = rn_lds + sp * RN_ROW + 16 * sg;
        *reinterpret_cast<rn_h8 *>(d) = hi;
        *reinterpret_cast<rn_h8 *>(d + HALF) = lo;
    };

    // A operand: tile i = output channels co0 + 16 i + li, K values 8 lk .. 8 lk + 7 of the step's line
    const char *__restrict__ wrow = a.w + ((size_t)(co0 + li) * steps) * 128 + lk * 16;
    const size_t wtile = (size_t)16 * steps * 128;

    rn_f4 acc[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[i][j] = (rn_f4){0.f, 0.f, 0.f, 0.f};

    gload(0);
    for (int s = 0; s < steps; ++s) {
        rn_h8 wh[MI], wl[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            wh[i] = *reinterpret_cast<const rn_h8 *>(wrow + i * wtile + (size_t)s * 128);
            wl[i] = *reinterpret_cast<const rn_h8 *>(wrow + i * wtile + (size_t)s * 128 + 64);
        }
        lstore();
        __syncthreads();
        if (s + 1 < steps)
            gload(s + 1);
        const char *S = rn_lds;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const char *b = S + (16 * j + li) * RN_ROW + 16 * lk;
            const rn_h8 xh = *reinterpret_cast<const rn_h8 *>(b);
            const rn_h8 xl = *reinterpret_cast<const rn_h8 *>(b + HALF);
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

    // epilogue: accumulator tile (i, j) holds output channels co0 + 16 i + 4 lk + r (r = register) of pixel q0 + 16 j + li
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = q0 + 16 * j + li;
        if (q >= HWo)
            continue;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = co0 + 16 * i + 4 * lk + r;
                const size_t o = ((size_t)n * a.Cout + co) * HWo + q;
                float v = __builtin_fmaf(acc[i][j][r], unscale, a.bias ? a.bias[co] : 0.f);
                if (a.res)
                    v += a.res[o];
                if (a.relu)
                    v = v < 0.f ? 0.f : v;
                a.out[o] = v;
            }
    }
}

extern "C" int rac_resnet_conv_fwd(const rac_resnet_conv *d, void *stream)
{
    const char *what = "rac_resnet_conv_fwd";
    RAC_CHECK_ARG(d, "%s: null pointer (descriptor)", what);
    RAC_CHECK_ARG(d->ksize == 1 || d->ksize == 3, "%s: ksize=%d (1 or 3)", what, d->ksize);
    RAC_CHECK_ARG(d->stride == 1 || d->stride == 2, "%s: stride=%d (1 or 2)", what, d->stride);
    RAC_CHECK_ARG(d->Cin >= 32 && d->Cin % 32 == 0 && d->Cin <= 2048, "%s: Cin=%d (a multiple of 32, at most 2048)", what, d->Cin);
    RAC_CHECK_ARG(d->Cout >= 64 && d->Cout % 64 == 0 && d->Cout <= 2048, "%s: Cout=%d (a multiple of 64, at most 2048)", what, d->Cout);
    RAC_CHECK_ARG(d->N >= 1 && d->H >= 1 && d->W >= 1 && (long)d->H * d->W < (1l << 30), "%s: N=%d H=%d W=%d must be positive", what,
                  d->N, d->H, d->W);
    RAC_CHECK_ARG(d->in && d->w_image && d->amax_parts && d->out, "%s: null pointer", what);
    RAC_CHECK_ARG((reinterpret_cast<uintptr_t>(d->w_image) & 15) == 0, "%s: w_image must be 16-byte aligned", what);
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(d->in) | reinterpret_cast<uintptr_t>(d->out) | reinterpret_cast<uintptr_t>(d->residual) |
                    reinterpret_cast<uintptr_t>(d->bias) | reinterpret_cast<uintptr_t>(d->amax_parts)) & 3) == 0,
                  "%s: in / residual / bias / amax_parts / out must be 4-byte aligned", what);
    RnConvArgs a;
    a.in = d->in; a.w = reinterpret_cast<const char *>(d->w_image); a.bias = d->bias; a.res = d->residual; a.parts = d->amax_parts;
    a.out = d->out; a.w_alpha = d->w_alpha; a.relu = d->relu;
    a.H = d->H; a.W = d->W; a.Cin = d->Cin; a.Cout = d->Cout; a.ksize = d->ksize; a.stride = d->stride; a.pad = d->ksize / 2;
    a.Ho = (d->H + 2 * a.pad - d->ksize) / d->stride + 1;
    a.Wo = (d->W + 2 * a.pad - d->ksize) / d->stride + 1;
    // 256 output channels per workgroup (the pixel tile is split once per 256 channels) where that still gives every CU a workgroup,
    // then 128, then 64: a function of the shapes alone
    const long ptiles = (long)d->N * ((a.Ho * a.Wo + 63) / 64);
    int mi = 1;
    for (int c = 4; c > 1; c >>= 1)
        if (d->Cout % (64 * c) == 0 && ptiles * (d->Cout / (64 * c)) >= 256) {
            mi = c;
            break;
        }
    a.cblocks = d->Cout / (64 * mi);
    const long wgs = ptiles * a.cblocks;
    RAC_CHECK_ARG(wgs < (1l << 31), "%s: %ld workgroups", what, wgs);
    const dim3 grid((unsigned)wgs);
    hipStream_t st = (hipStream_t)stream;
    if (mi == 4) hipLaunchKernelGGL(rn_conv_kernel<4>, grid, dim3(256), 0, st, a);
    else if (mi == 2) hipLaunchKernelGGL(rn_conv_kernel<2>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(rn_conv_kernel<1>, grid, dim3(256), 0, st, a);
    return rac_launch_status(what);
}

// ------------------------------------------------------------------------------------------------ stem
struct RnStemArgs {
    const float *img;   // [N][3][H][W]
    const float *w;     // [147][64], tap (ci * 7 + ky) * 7 + kx
    const float *bias;  // [64]
    float *conv;        // [N][64][Hc][Wc]
    float *out;         // [N][64][Hp][Wp]
    float mean[3], std[3];
    int perm[3];
    int norm, H, W, Hc, Wc, Hp, Wp, tiles_x, tiles_y;
};

__global__ __launch_bounds__(256) void rn_stem_kernel(const RnStemArgs a)
{
    __shared__ __attribute__((aligned(16))) float sw[RN_STEM_TAPS * RN_STEM_C];
    __shared__ float sx[3 * RN_STEM_PATCH * RN_STEM_PATCH];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int tpi = a.tiles_x * a.tiles_y;
    const int n = blockIdx.x / tpi, t = blockIdx.x - n * tpi;
    const int oy0 = (t / a.tiles_x) * 16, ox0 = (t % a.tiles_x) * 16;
    for (int i = tid; i < RN_STEM_TAPS * RN_STEM_C; i += 256)
        sw[i] = a.w[i];
    const size_t HW = (size_t)a.H * a.W;
    for (int i = tid; i < 3 * RN_STEM_PATCH * RN_STEM_PATCH; i += 256) {
        const int c = i / (RN_STEM_PATCH * RN_STEM_PATCH), r = i - c * RN_STEM_PATCH * RN_STEM_PATCH;
        const int py = r / RN_STEM_PATCH, px = r - py * RN_STEM_PATCH;
        const int ih = oy0 * 2 - 3 + py, iw = ox0 * 2 - 3 + px;
        float v = 0.f;
        if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) {
            const int cs = a.norm ? a.perm[c] : c;
            v = a.img[((size_t)n * 3 + cs) * HW + (size_t)ih * a.W + iw];
            if (a.norm)
                v = __fdiv_rn(v - a.mean[c], a.std[c]);
        }
        sx[i] = v;
    }
    __syncthreads();
    float acc[RN_STEM_C];
#pragma unroll
    for (int co = 0; co < RN_STEM_C; ++co)
        acc[co] = 0.f;
#pragma unroll 1
    for (int c = 0; c < 3; ++c)
#pragma unroll 1
        for (int ky = 0; ky < 7; ++ky) {
            const float *xr = sx + (c * RN_STEM_PATCH + 2 * ty + ky) * RN_STEM_PATCH + 2 * tx;
            const float *wr = sw + (c * 7 + ky) * 7 * RN_STEM_C;
#pragma unroll
            for (int kx = 0; kx < 7; ++kx) {
                const float x = xr[kx];
#pragma unroll
                for (int c4 = 0; c4 < RN_STEM_C / 4; ++c4) {
                    const rn_f4 w4 = *reinterpret_cast<const rn_f4 *>(wr + kx * RN_STEM_C + 4 * c4);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        acc[4 * c4 + r] = __builtin_fmaf(x, w4[r], acc[4 * c4 + r]);
                }
            }
        }
    const int oy = oy0 + ty, ox = ox0 + tx;
    if (oy < a.Hc && ox < a.Wc) {
        const size_t plane = (size_t)a.Hc * a.Wc;
        float *o = a.conv + (size_t)n * RN_STEM_C * plane + (size_t)oy * a.Wc + ox;
#pragma unroll
        for (int co = 0; co < RN_STEM_C; ++co) {
            const float v = acc[co] + a.bias[co];
            o[(size_t)co * plane] = v < 0.f ? 0.f : v;
        }
    }
}

__global__ __launch_bounds__(256) void rn_pool_kernel(const RnStemArgs a, long total)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total)
        return;
    const int pw = (int)(i % a.Wp);
    const long r = i / a.Wp;
    const int ph = (int)(r % a.Hp);
    const long nc = r / a.Hp;                            // n * 64 + c
    const float *src = a.conv + (size_t)nc * a.Hc * a.Wc;
    float m = -INFINITY;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int y = 2 * ph + dy, x = 2 * pw + dx;
            if (y >= 0 && y < a.Hc && x >= 0 && x < a.Wc) {
                const float v = src[(size_t)y * a.Wc + x];
                m = (v > m || v != v) ? v : m;
            }
        }
    a.out[i] = m;
}

extern "C" int rac_resnet_stem_fwd(const rac_resnet_stem *d, void *stream)
{
    const char *what = "rac_resnet_stem_fwd";
    RAC_CHECK_ARG(d, "%s: null pointer (descriptor)", what);
    RAC_CHECK_ARG(d->N >= 1 && d->H >= 1 && d->W >= 1 && d->H <= (1 << 20) && d->W <= (1 << 20), "%s: N=%d H=%d W=%d must be positive",
                  what, d->N, d->H, d->W);
    RAC_CHECK_ARG(d->img && d->w && d->bias && d->conv && d->out, "%s: null pointer", what);
    RAC_CHECK_ARG((reinterpret_cast<uintptr_t>(d->w) & 15) == 0, "%s: w must be 16-byte aligned", what);
    RnStemArgs a;
    a.img = d->img; a.w = d->w; a.bias = d->bias; a.conv = d->conv; a.out = d->out;
    a.norm = d->norm != 0;
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = d->mean[c]; a.std[c] = d->std[c]; a.perm[c] = d->perm[c];
        RAC_CHECK_ARG(!a.norm || (a.perm[c] >= 0 && a.perm[c] < 3), "%s: perm[%d]=%d", what, c, a.perm[c]);
    }
    a.H = d->H; a.W = d->W;
    a.Hc = (d->H + 6 - 7) / 2 + 1; a.Wc = (d->W + 6 - 7) / 2 + 1;
    a.Hp = (a.Hc + 2 - 3) / 2 + 1; a.Wp = (a.Wc + 2 - 3) / 2 + 1;
    a.tiles_x = (a.Wc + 15) / 16; a.tiles_y = (a.Hc + 15) / 16;
    const long wgs = (long)d->N * a.tiles_x * a.tiles_y;
    const long total = (long)d->N * RN_STEM_C * a.Hp * a.Wp;
    RAC_CHECK_ARG(wgs < (1l << 31) && (total + 255) / 256 < (1l << 31), "%s: %ld workgroups", what, wgs);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(rn_stem_kernel, dim3((unsigned)wgs), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rn_pool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a, total);
    return rac_launch_status(what);
}
