// fpn_lateral_bwd.hip -- backward of the image necks' lateral stage (fpn_lateral.hip): the top-down add and the weight / bias gradients
// of the 1x1 lateral convolution (gfx950).  The data gradient is the forward's kernel on the image of W^T (rac_fpn_lateral_dgrad,
// fpn_lateral.hip).
//
//   rac_fpn_merge_bwd       G[n][c][p] = A[n][c][p] + sum over q with src(q) == p of Gfine[n][c][q]
//   rac_fpn_lateral_wgrad   dW[co][ci] = sum_{n,p} G[n][co][p] * x[n][ci][p],   db[co] = sum_{n,p} G[n][co][p]
//
// Merge.  src is the forward's legacy 'nearest' rule, non-decreasing along an axis: the fine pixels that read coarse index i are one
// contiguous range [start[i], start[i + 1]) per axis, given by two host-built int32 tables (necks.nearest_children: the same float32
// arithmetic as the forward's).  One thread per element of G gathers its children row-major and adds them to A in that order: exact
// float additions in a fixed order, no scatter, no atomics.  The ranges are clamped to the fine map, so a wrong table cannot make
// the kernel read outside it.
//
// Weight gradient.  Both operands are channel-first, so the reduction index (the pixel) is the contiguous one: a lane's MFMA fragment
// -- 8 consecutive k of one row (A: G's channel co) or one column (B: x's channel ci) -- is 8 consecutive pixels of one channel, and
// the LDS image needs no transpose.  The split-K scheme, its per-channel scale, LDS image, epilogue and reduce launch are
// wgrad_splitk.h's (shared with resnet_bwd.hip); this file has the loader, the tile and the bias sums.  A workgroup owns a K range
// and a tile of all 256 co x CT ci (CT = 128, or 64 for narrow levels); workspace [k_splits][256][Cin].
// Arithmetic as in the forward: v * 2^e = hi + lo (two f16), the three leading products per K step in v_mfma_f32_16x16x32_f16, fp32
// accumulate.  No pass over the maps for a global maximum, nothing the host has to read, and a range of small gradients keeps its
// 22 bits beside a range of large ones.  The second walk finds the range in L2 / the Infinity Cache.
// Workgroup = 256 threads = 4 waves; wave w owns co 64 w .. 64 w + 63 x the CT ci = 4 x NJ MFMA tiles.  Per unit the (256 + CT) x 32
// fp32 block goes global -> registers (one unit ahead, under the MFMAs) -> (scale, split) -> LDS.  Pixels past the image are loaded
// from a clamped address and replaced by zero; ci rows past Cin (a last tile of fewer than
// CT) re-read row Cin - 1 and are not stored.  One LDS stage, two barriers per unit; two workgroups share a CU.
// db: the threads that stage G add their values in fp32 during the first walk (tile 0's workgroups only), per range, in a fixed order.
#include "wgrad_splitk.h"

#define FB_COUT 256

// ------------------------------------------------------------------------------------------------ merge
__global__ __launch_bounds__(256) void fpn_merge_bwd_kernel(const float *__restrict__ a, const float *__restrict__ gf,
                                                            const int *__restrict__ rs, const int *__restrict__ cs,
                                                            float *__restrict__ g, long total, int H, int W, int fh, int fw)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total)
        return;
    const int HW = H * W;
    const long plane = e / HW;
    const int p = (int)(e - plane * HW), h = p / W, w = p - h * W;
    float s = a ? a[e] : 0.f;
    if (gf) {
        const int r0 = max(rs[h], 0), r1 = min(rs[h + 1], fh), c0 = max(cs[w], 0), c1 = min(cs[w + 1], fw);
        const float *__restrict__ src = gf + plane * ((long)fh * fw);
        for (int r = r0; r < r1; ++r)
            for (int c = c0; c < c1; ++c)
                s += src[(long)r * fw + c];
    }
    g[e] = s;
}

extern "C" int rac_fpn_merge_bwd(const float *a, const float *gfine, const int *row_start, const int *col_start, float *g, int N, int C,
                                 int H, int W, int fine_h, int fine_w, void *stream)
{
    const char *what = "rac_fpn_merge_bwd";
    RAC_CHECK_ARG(N >= 0 && C >= 1 && H >= 1 && W >= 1 && (long)H * W < (1l << 30), "%s: N=%d C=%d H=%d W=%d", what, N, C, H, W);
    RAC_CHECK_ARG(!gfine || (fine_h >= H && fine_w >= W && (long)fine_h * fine_w < (1l << 30)),
                  "%s: the level %dx%d must be no larger than the finer one %dx%d", what, H, W, fine_h, fine_w);
    if (N == 0)
        return 0;
    RAC_CHECK_ARG(g && (a || gfine) && (!gfine || (row_start && col_start)), "%s: null pointer", what);
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(gfine) | reinterpret_cast<uintptr_t>(g) |
                    reinterpret_cast<uintptr_t>(row_start) | reinterpret_cast<uintptr_t>(col_start)) & 3) == 0,
                  "%s: pointers must be 4-byte aligned", what);
    const long total = (long)N * C * H * W, blocks = (total + 255) / 256;
    RAC_CHECK_ARG(blocks < (1l << 31), "%s: %ld workgroups", what, blocks);
    hipLaunchKernelGGL(fpn_merge_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a, gfine, row_start, col_start,
                       g, total, H, W, fine_h, fine_w);
    return rac_launch_status(what);
}

// ------------------------------------------------------------------------------------------------ weight and bias gradients
struct FpnWgradArgs {
    const float *g;      // [N][256][HW]
    const float *x;      // [N][Cin][HW]
    float *ws;           // [k_splits][256][Cin] partial sums
    float *wsb;          // [k_splits][256] partial bias sums, or null
    int Cin, HW, upi, units, per, ntiles;      // upi: units of 32 pixels per image; per: units per K range
};

// NJ: 16-channel MFMA tiles of ci per workgroup (8: CT = 128, 4: CT = 64).  VEC: 16-byte loads (H*W % 4 == 0, g and x 16-byte aligned).
template <int NJ, bool VEC>
__global__ __launch_bounds__(256, 2) void fpn_lateral_wgrad_kernel(const FpnWgradArgs a)
{
    constexpr int CT = 16 * NJ;
    constexpr int ROWS = FB_COUT + CT;      // LDS rows: G's 256 channels, then the tile's CT channels of x
    constexpr int NP = ROWS / 64;           // staging passes of 64 rows
    constexpr int HALF = ROWS * 64;         // bytes of the hi image (the lo image follows)
    __shared__ __attribute__((aligned(16))) char fb_lds[2 * HALF];
    __shared__ float fb_unscale[ROWS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int HW = a.HW, Cin = a.Cin;
    const int split = blockIdx.x / a.ntiles, ct = blockIdx.x - split * a.ntiles;
    const int u0 = split * a.per, u1 = min(u0 + a.per, a.units);

    // staging role: pass j = row 64 j + s_r of the block, pixels 8 s_q .. 8 s_q + 7 of the unit
    const int s_r = tid >> 2, s_q = tid & 3;
    int xrow[NP - 4];
#pragma unroll
    for (int j = 0; j < NP - 4; ++j)
        xrow[j] = min(CT * ct + 64 * j + s_r, Cin - 1);
    auto gload = [&](int u, rac_f4v *rx) {
        const int n = u / a.upi, p0 = (u - n * a.upi) * 32 + 8 * s_q;
        const float *__restrict__ gn = a.g + (size_t)n * FB_COUT * HW;
        const float *__restrict__ xn = a.x + (size_t)n * Cin * HW;
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const float *row = j < 4 ? gn + (size_t)(64 * j + s_r) * HW : xn + (size_t)xrow[j < 4 ? 0 : j - 4] * HW;
            if (VEC) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int p = p0 + 4 * h;
                    const rac_f4v v = *reinterpret_cast<const rac_f4v *>(row + min(p, HW - 4));
                    rx[2 * j + h] = p < HW ? v : (rac_f4v){0.f, 0.f, 0.f, 0.f};
                }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int p = p0 + e;
                    const float v = row[min(p, HW - 1)];
                    rx[2 * j + (e >> 2)][e & 3] = p < HW ? v : 0.f;
                }
            }
        }
    };

    // ---- first walk: per-channel maxima over this K range (and the bias sums, by the workgroups of tile 0)
    const bool do_bias = a.wsb != nullptr && ct == 0;
    float mx[NP];
    rac_f4v bs[4];
#pragma unroll
    for (int j = 0; j < NP; ++j)
        mx[j] = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        bs[j] = (rac_f4v){0.f, 0.f, 0.f, 0.f};
    for (int u = u0; u < u1; ++u) {
        rac_f4v r[2 * NP];
        gload(u, r);
#pragma unroll
        for (int j = 0; j < NP; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e)
                mx[j] = fmaxf(mx[j], fabsf(r[2 * j + (e >> 2)][e & 3]));
        if (do_bias) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bs[j] += r[2 * j];
                bs[j] += r[2 * j + 1];
            }
        }
    }
    float sc[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        float us;
        sc[j] = wg_row_scale(mx[j], us);
        if (s_q == 0)
            fb_unscale[64 * j + s_r] = us;
    }
    if (do_bias) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float t = wg_row_sum((bs[j][0] + bs[j][1]) + (bs[j][2] + bs[j][3]));
            if (s_q == 0)
                a.wsb[(size_t)split * FB_COUT + 64 * j + s_r] = t;
        }
    }

    // ---- second walk: the products.  Wave w owns co 64 w .. 64 w + 63 x the CT ci = 4 x NJ MFMA tiles.
    rac_f4v acc[4][NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            acc[i][j] = (rac_f4v){0.f, 0.f, 0.f, 0.f};
    const int a_off = wg_frag_off(64 * wave, li, lk), b_off = wg_frag_off(FB_COUT, li, lk);
    rac_f4v rx[2 * NP];
    gload(u0, rx);
    for (int u = u0; u < u1; ++u) {
#pragma unroll
        for (int j = 0; j < NP; ++j)
            wg_stage(fb_lds, HALF, 64 * j + s_r, s_q, sc[j], [&](int e) { return rx[2 * j + (e >> 2)][e & 3]; });
        __syncthreads();
        gload(u + 1 < u1 ? u + 1 : u, rx);      // (past the end the last unit again: unconditional code)
        __builtin_amdgcn_sched_barrier(0);      // (the conversion of the next unit, and the wait for these loads, stay behind the MFMAs)
        wg_products<3>(fb_lds, HALF, a_off, b_off, acc);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();      // every wave has read the stage: the next unit may overwrite it
    }

    wg_store(a.ws + (size_t)split * FB_COUT * Cin, fb_unscale, FB_COUT, acc, CT * ct, Cin, wave, li, lk);
}

extern "C" int rac_fpn_lateral_wgrad(const float *g, const float *x, float *workspace, float *dw, float *db, int N, int Cin, int H,
                                     int W, int Cout, int k_splits, void *stream)
{
    const char *what = "rac_fpn_lateral_wgrad";
    RAC_CHECK_ARG(Cout == FB_COUT, "%s: built for %d output channels (got %d)", what, FB_COUT, Cout);
    RAC_CHECK_ARG(Cin >= 32 && Cin % 32 == 0 && Cin <= 2048, "%s: Cin=%d (a multiple of 32 from 32 to 2048)", what, Cin);
    RAC_CHECK_ARG(N >= 1 && H >= 1 && W >= 1 && (long)H * W < (1l << 30), "%s: N=%d H=%d W=%d", what, N, H, W);
    WgSplit ks;
    if (const int rc = wg_split(what, "H", "W", N, H, W, k_splits, g, x, workspace, dw, db, ks))
        return rc;
    const int HW = H * W;
    const bool wide = Cin >= 128;
    const int ctile = wide ? 128 : 64, ntiles = (Cin + ctile - 1) / ctile;
    RAC_CHECK_ARG((long)k_splits * ntiles < (1l << 31), "%s: %ld workgroups", what, (long)k_splits * ntiles);
    FpnWgradArgs a;
    a.g = g; a.x = x; a.ws = workspace;
    a.wsb = db ? workspace + (size_t)k_splits * FB_COUT * Cin : nullptr;
    a.Cin = Cin; a.HW = HW; a.upi = ks.upi; a.units = ks.units; a.per = ks.per; a.ntiles = ntiles;
    const bool vec = HW % 4 == 0 && ((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(x)) & 15) == 0;
    const dim3 grid((unsigned)(k_splits * ntiles));
    hipStream_t st = (hipStream_t)stream;
    if (wide && vec) hipLaunchKernelGGL((fpn_lateral_wgrad_kernel<8, true>), grid, dim3(256), 0, st, a);
    else if (wide) hipLaunchKernelGGL((fpn_lateral_wgrad_kernel<8, false>), grid, dim3(256), 0, st, a);
    else if (vec) hipLaunchKernelGGL((fpn_lateral_wgrad_kernel<4, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((fpn_lateral_wgrad_kernel<4, false>), grid, dim3(256), 0, st, a);
    wg_reduce(workspace, a.wsb, dw, db, FB_COUT, Cin, 1, k_splits, st);
    return rac_launch_status(what);
}
