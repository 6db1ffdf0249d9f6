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
// from a pass of its own (rn_absmax_kernel: RAC_AMAX_PARTS partial maxima per image, combined by every workgroup of the convolution -- a maximum
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
// The same kernel source is the convolution's data gradient (template Rule, rac_resnet_conv_dgrad below): the roles of Cin and Cout
// exchanged, the image of W^T with the taps flipped as the weights, g as the activations with one scale per image; the two rules differ
// in which source pixel a tap reads and in the epilogue.  The rest of the backward is resnet_bwd.hip.
//
// rn_stem_kernel: exact fp32 (an fmaf chain over (ci, ky, kx) in ascending order per output).  K = 147 is no multiple of the MFMA's 32
// and the layer is bound by its 554 MB of output at the f8 shapes, not by arithmetic.  A workgroup owns 16 x 16 convolution outputs of
// one image x all 64 channels: weights [147][64] and the 37 x 37 x 3 input patch in LDS, the optional input normalisation
// (x[perm[c]] - mean[c]) / std[c] (IEEE division) applied while the patch is staged; padding stays zero.  rn_pool_kernel then takes the
// maximum of the valid pixels of each 3x3 / stride 2 / pad 1 window.
// No atomics, nothing read back, every sum in one fixed order, launch geometry from the shapes alone; 64-bit index arithmetic.
#include "split_f16.h"

#define RN_ROW 80         // bytes per LDS pixel row: 32 f16 + 16 bytes of padding (spreads the 16-byte reads over the banks)
#define RN_STEM_C 64
#define RN_STEM_TAPS 147
#define RN_STEM_PATCH 37  // (16 - 1) * 2 + 7

// ------------------------------------------------------------------------------------------------ per-image maximum
__global__ __launch_bounds__(256) void rn_absmax_kernel(const float *__restrict__ x, float *__restrict__ parts, long per_image)
{
    __shared__ unsigned red[4];
    const int n = blockIdx.y, part = blockIdx.x, tid = threadIdx.x;
    const long len = (per_image + RAC_AMAX_PARTS - 1) / RAC_AMAX_PARTS;
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
        parts[(size_t)n * RAC_AMAX_PARTS + part] = __uint_as_float(max(max(red[0], red[1]), max(red[2], red[3])));
}

extern "C" int rac_resnet_absmax_fwd(const float *x, float *parts, int N, int64_t per_image, void *stream)
{
    const char *what = "rac_resnet_absmax_fwd";
    RAC_CHECK_ARG(N >= 1 && N <= 65535 && per_image >= 1, "%s: N=%d per_image=%ld", what, N, (long)per_image);
    RAC_CHECK_ARG(x && parts, "%s: null pointer", what);
    hipLaunchKernelGGL(rn_absmax_kernel, dim3(RAC_AMAX_PARTS, (unsigned)N), dim3(256), 0, (hipStream_t)stream, x, parts, (long)per_image);
    return rac_launch_status(what);
}

// ------------------------------------------------------------------------------------------------ Bottleneck convolution
// One kernel for the forward and the data gradient: source map -> destination map through a weight image with the destination's
// channels as rows.  Forward: source = in (H x W, Cin), destination = out (Ho x Wo, Cout).  Data gradient: source = g (Ho x Wo, Cout),
// destination = dx (H x W, Cin), the image that of W^T with the taps flipped.
struct RnConvArgs {
    const float *src;     // [N][Cs][Hs*Ws]
    const char *w;        // [Cd][steps][hi 32 | lo 32] f16, step = tap * (Cs / 32) + chunk
    const float *e0;      // forward: bias [Cd];  data gradient: add [N][Cd][Hd*Wd];  or null
    const float *e1;      // forward: residual [N][Cd][Hd*Wd];  data gradient: mask [N][Cd][Hd*Wd];  or null
    const float *parts;   // [N][RAC_AMAX_PARTS] partial maxima of src
    float *dst;           // [N][Cd][Hd*Wd]
    float w_alpha;
    int relu, Hs, Ws, Hd, Wd, Cs, Cd, ksize, stride, pad, cblocks;
};

// What the two directions differ in.  tap: the source pixel (sh, sw) that tap (ky, kx) of destination pixel (dh, dw) reads, and
// whether there is one for a thread whose pixel is `live`, i.e. inside the map (the kernel clamps the coordinates and stages a zero where
// there is none).  The flag is formed before the coordinates are written out: the other way round hipcc merges two of its compares
// behind a v_or_b32 in the K loop's staging code, 1.2 % on layer4 at 6 images.  store: the value stored for an
// accumulator of channel c at element o of the destination.
struct RnForward {
    static constexpr bool dgrad = false;
    static __device__ __forceinline__ bool tap(const RnConvArgs &a, bool live, int dh, int dw, int ky, int kx, int &sh, int &sw)
    {
        const int ih = dh * a.stride + ky - a.pad, iw = dw * a.stride + kx - a.pad;
        const bool valid = live && ih >= 0 && ih < a.Hs && iw >= 0 && iw < a.Ws;
        sh = ih, sw = iw;
        return valid;
    }
    static __device__ __forceinline__ float store(const RnConvArgs &a, float acc, float unscale, int c, size_t o)
    {
        float v = __builtin_fmaf(acc, unscale, a.e0 ? a.e0[c] : 0.f);
        if (a.e1)
            v += a.e1[o];
        if (a.relu)
            v = v < 0.f ? 0.f : v;
        return v;
    }
};
// At stride 1 the forward itself.  At stride 2 pixel p reads tap t' at n = p + t' - pad only where both coordinates of n are even and
// n / 2 lies inside g.  The epilogue adds `add` (the identity branch, an outside gradient) and applies the ReLU backward of the layer in
// front (mask = the convolution's own post-ReLU input): a masked element is +0 exactly.
struct RnDgrad {
    static constexpr bool dgrad = true;
    static __device__ __forceinline__ bool tap(const RnConvArgs &a, bool live, int dh, int dw, int ky, int kx, int &sh, int &sw)
    {
        const int sft = a.stride - 1;                    // stride 1 or 2: a shift and a parity mask
        const int nh = dh + ky - a.pad, nw = dw + kx - a.pad;
        const int qh = nh >> sft, qw = nw >> sft;
        const bool valid = live && nh >= 0 && nw >= 0 && ((nh | nw) & sft) == 0 && qh < a.Hs && qw < a.Ws;
        sh = qh, sw = qw;
        return valid;
    }
    static __device__ __forceinline__ float store(const RnConvArgs &a, float acc, float unscale, int c, size_t o)
    {
        float v = acc * unscale;
        if (a.e0)
            v += a.e0[o];
        if (a.e1)
            v = a.e1[o] <= 0.f ? 0.f : v;
        return v;
    }
};

template <class Rule, int MI>
__global__ __launch_bounds__(256) void rn_conv_kernel(const RnConvArgs a)
{
    constexpr int HALF = 64 * RN_ROW;
    __shared__ __attribute__((aligned(16))) char rn_lds[2 * HALF];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int cb = blockIdx.x % a.cblocks;
    const long pt = blockIdx.x / a.cblocks;              // pixel tile over all images
    const int HWd = a.Hd * a.Wd, tiles = (HWd + 63) / 64;
    const int n = (int)(pt / tiles), q0 = (int)(pt - (long)n * tiles) * 64;
    const int c0 = cb * 64 * MI + wave * 16 * MI;
    const int chunks = a.Cs >> 5, steps = a.ksize * a.ksize * chunks;
    const size_t HWs = (size_t)a.Hs * a.Ws;

    // the image's scale, by every wave
    const float sc = rac_act_scale(rac_wave_amax(a.parts + (size_t)n * RAC_AMAX_PARTS, lane));
    const float unscale = a.w_alpha / sc;                // both powers of two: exact

    // staging role: pixel sp of the tile, channels 8 sg .. 8 sg + 7 of the step's 32
    const int sp = tid & 63, sg = tid >> 6;
    const bool live = q0 + sp < HWd;
    const int qc = live ? q0 + sp : HWd - 1;
    const int dh = qc / a.Wd, dw = qc - dh * a.Wd;
    const float *__restrict__ xin = a.src + ((size_t)n * a.Cs + 8 * sg) * HWs;
    float rx[8];
    bool rvalid = false;
    auto gload = [&](int s) {
        const int tap = s / chunks, c = s - tap * chunks;
        const int ky = tap / a.ksize, kx = tap - ky * a.ksize;
        int sh, sw;
        rvalid = Rule::tap(a, live, dh, dw, ky, kx, sh, sw);
        const int shc = min(max(sh, 0), a.Hs - 1), swc = min(max(sw, 0), a.Ws - 1);
        const float *p = xin + (size_t)c * 32 * HWs + (size_t)shc * a.Ws + swc;
#pragma unroll
        for (int e = 0; e < 8; ++e)
            rx[e] = p[(size_t)e * HWs];
    };
    auto lstore = [&]() {
        rac_h8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float v = rvalid ? rx[e] * sc : 0.f;
            hi[e] = (_Float16)v;
            lo[e] = (_Float16)(v - (float)hi[e]);
        }
        char *d = rn_lds + sp * RN_ROW + 16 * sg;
        *reinterpret_cast<rac_h8 *>(d) = hi;
        *reinterpret_cast<rac_h8 *>(d + HALF) = lo;
    };

    // A operand: tile i = destination channels c0 + 16 i + li, K values 8 lk .. 8 lk + 7 of the step's line
    const char *__restrict__ wrow = a.w + ((size_t)(c0 + li) * steps) * 128 + lk * 16;
    const size_t wtile = (size_t)16 * steps * 128;

    rac_f4v acc[MI][4];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc[i][j] = (rac_f4v){0.f, 0.f, 0.f, 0.f};

    gload(0);
    for (int s = 0; s < steps; ++s) {
        rac_h8 wh[MI], wl[MI];
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            wh[i] = *reinterpret_cast<const rac_h8 *>(wrow + i * wtile + (size_t)s * 128);
            wl[i] = *reinterpret_cast<const rac_h8 *>(wrow + i * wtile + (size_t)s * 128 + 64);
        }
        lstore();
        __syncthreads();
        if (s + 1 < steps)
            gload(s + 1);
        const char *S = rn_lds;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const char *b = S + (16 * j + li) * RN_ROW + 16 * lk;
            const rac_h8 xh = *reinterpret_cast<const rac_h8 *>(b);
            const rac_h8 xl = *reinterpret_cast<const rac_h8 *>(b + HALF);
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

    // epilogue: accumulator tile (i, j) holds destination channels c0 + 16 i + 4 lk + r (r = register) of pixel q0 + 16 j + li
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int q = q0 + 16 * j + li;
        if (q >= HWd)
            continue;
#pragma unroll
        for (int i = 0; i < MI; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = c0 + 16 * i + 4 * lk + r;
                const size_t o = ((size_t)n * a.Cd + c) * HWd + q;
                a.dst[o] = Rule::store(a, acc[i][j][r], unscale, c, o);
            }
    }
}

// The checks, the tile-width rule and the launch of both directions.  The caller has set a's pointers, w_alpha, relu, ksize and stride;
// H x W is the forward's input map, Ho x Wo its output (the forward derives it, the data gradient's is checked); `maps` names the
// 4-byte aligned pointers in the message.
template <class Rule>
static int rn_conv_launch(const char *what, const char *maps, RnConvArgs a, int N, int Cin, int Cout, int H, int W, int Ho, int Wo,
                          void *stream)
{
    constexpr bool DG = Rule::dgrad;
    constexpr int cin_unit = DG ? 64 : 32, cout_unit = DG ? 32 : 64;      // the destination's tiles of 64, the source's K steps of 32
    RAC_CHECK_ARG(a.ksize == 1 || a.ksize == 3, "%s: ksize=%d (1 or 3)", what, a.ksize);
    RAC_CHECK_ARG(a.stride == 1 || a.stride == 2, "%s: stride=%d (1 or 2)", what, a.stride);
    RAC_CHECK_ARG(Cin >= cin_unit && Cin % cin_unit == 0 && Cin <= 2048, "%s: Cin=%d (a multiple of %d, at most 2048)", what, Cin,
                  cin_unit);
    RAC_CHECK_ARG(Cout >= cout_unit && Cout % cout_unit == 0 && Cout <= 2048, "%s: Cout=%d (a multiple of %d, at most 2048)", what, Cout,
                  cout_unit);
    RAC_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && (long)H * W < (1l << 30), "%s: N=%d H=%d W=%d must be positive", what, N, H, W);
    if (!DG)
        Ho = rac_conv_out_size(H, a.ksize, a.stride), Wo = rac_conv_out_size(W, a.ksize, a.stride);
    RAC_CHECK_ARG(Ho >= 1 && Wo >= 1 && Ho == rac_conv_out_size(H, a.ksize, a.stride) && Wo == rac_conv_out_size(W, a.ksize, a.stride),
                  "%s: H=%d W=%d does not map to Ho=%d Wo=%d (ksize %d, stride %d)", what, H, W, Ho, Wo, a.ksize, a.stride);
    RAC_CHECK_ARG(a.src && a.w && a.parts && a.dst, "%s: null pointer", what);
    RAC_CHECK_ARG((reinterpret_cast<uintptr_t>(a.w) & 15) == 0, "%s: w_image must be 16-byte aligned", what);
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(a.src) | reinterpret_cast<uintptr_t>(a.dst) | reinterpret_cast<uintptr_t>(a.e0) |
                    reinterpret_cast<uintptr_t>(a.e1) | reinterpret_cast<uintptr_t>(a.parts)) & 3) == 0,
                  "%s: %s must be 4-byte aligned", what, maps);
    a.pad = a.ksize / 2;
    a.Hs = DG ? Ho : H; a.Ws = DG ? Wo : W; a.Cs = DG ? Cout : Cin;
    a.Hd = DG ? H : Ho; a.Wd = DG ? W : Wo; a.Cd = DG ? Cin : Cout;
    // 256 destination channels per workgroup (the pixel tile is split once per 256 channels) where that still gives every CU a
    // workgroup, then 128, then 64: a function of the shapes alone
    const long ptiles = (long)N * ((a.Hd * a.Wd + 63) / 64);
    int mi = 1;
    for (int c = 4; c > 1; c >>= 1)
        if (a.Cd % (64 * c) == 0 && ptiles * (a.Cd / (64 * c)) >= 256) {
            mi = c;
            break;
        }
    a.cblocks = a.Cd / (64 * mi);
    const long wgs = ptiles * a.cblocks;
    RAC_CHECK_ARG(wgs < (1l << 31), "%s: %ld workgroups", what, wgs);
    const dim3 grid((unsigned)wgs);
    hipStream_t st = (hipStream_t)stream;
    if (mi == 4) hipLaunchKernelGGL((rn_conv_kernel<Rule, 4>), grid, dim3(256), 0, st, a);
    else if (mi == 2) hipLaunchKernelGGL((rn_conv_kernel<Rule, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((rn_conv_kernel<Rule, 1>), grid, dim3(256), 0, st, a);
    return rac_launch_status(what);
}

extern "C" int rac_resnet_conv_fwd(const rac_resnet_conv *d, void *stream)
{
    const char *what = "rac_resnet_conv_fwd";
    RAC_CHECK_ARG(d, "%s: null pointer (descriptor)", what);
    RnConvArgs a;
    a.src = d->in; a.w = reinterpret_cast<const char *>(d->w_image); a.e0 = d->bias; a.e1 = d->residual; a.parts = d->amax_parts;
    a.dst = d->out; a.w_alpha = d->w_alpha; a.relu = d->relu; a.ksize = d->ksize; a.stride = d->stride;
    return rn_conv_launch<RnForward>(what, "in / residual / bias / amax_parts / out", a, d->N, d->Cin, d->Cout, d->H, d->W, 0, 0, stream);
}

// dx = the same kernel on the line image of W^T as [Cin][K], K = (flipped tap, co), with g as the activations.  The output size H x W
// is an argument (7 and 8 both map to 4) and is checked against the forward's formula.
extern "C" int rac_resnet_conv_dgrad(const rac_resnet_dgrad *d, void *stream)
{
    const char *what = "rac_resnet_conv_dgrad";
    RAC_CHECK_ARG(d, "%s: null pointer (descriptor)", what);
    RnConvArgs a;
    a.src = d->g; a.w = reinterpret_cast<const char *>(d->w_image); a.e0 = d->add; a.e1 = d->mask; a.parts = d->amax_parts;
    a.dst = d->out; a.w_alpha = d->w_alpha; a.relu = 0; a.ksize = d->ksize; a.stride = d->stride;
    return rn_conv_launch<RnDgrad>(what, "g / add / mask / amax_parts / out", a, d->N, d->Cin, d->Cout, d->H, d->W, d->Ho, d->Wo, stream);
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
                    const rac_f4v w4 = *reinterpret_cast<const rac_f4v *>(wr + kx * RN_STEM_C + 4 * c4);
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
