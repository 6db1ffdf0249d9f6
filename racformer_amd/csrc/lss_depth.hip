// lss_depth.hip -- what feeds and supervises the depth branch of LSSViewTransformerBEVDepth_racformer
// (models/necks/view_transformer_racformer.py:593-699, models/necks/focalloss.py:114-125 of the reference), gfx950.
//
//   ld_pool_kernel        radar / lidar depth map and RCS map [BN, H, W] -> per feature pixel the pooled depth, the quadratic
//                         depth bin and the RCS class; every full-resolution value is read once, straight from [BN, H, W]
//   ld_prior_kernel       the two index maps -> the channel-first tensor DepthNet concatenates behind its features:
//                         one-hot depth grid (D + 1 channels) | rcs_embedding column + bias (E channels); no one-hot input built
//   ld_prior_bwd_kernel   d weight / d bias of that embedding: per class, the pixels of a segment summed in ascending order
//   ld_prior_bwd_finish_kernel   the segments in ascending order
//   ld_loss_kernel        softmax focal loss of the depth logits against the bin labels per foreground pixel, its unscaled
//                         gradient in the same launch, one (sum, count) pair per workgroup of 64 pixels
//   ld_loss_finish_kernel the pairs in index order -> loss = weight * sum / max(1, count) and the scale weight / max(1, count)
//   ld_loss_bwd_kernel    grad_logits = unscaled * scale * grad_loss, all three on the device
//
// Every launch is sized by shapes, nothing is read back and no floating-point sum is atomic: capturable, bitwise reproducible.
#include "rac_common.h"

#define LD_MAX_DS 1024         // largest pooling block edge: ld_pool_kernel keeps one tile of max(256, ds) columns in LDS
#define LD_MAX_SEGS 8          // pixel segments of ld_prior_bwd_kernel (workgroups per embedding channel)
#define LD_EMPTY_DEPTH 1.0e5f
#define LD_EMPTY_RCS -1.0e5f

struct LdBins {
    float d_lo, d_bin;         // depth: lower bound, float32(2 (hi - lo) / (n (n + 1)))
    int d_n;
    float r_lo, r_off, r_bin;  // rcs: lower bound, float32(lo - bin), float32(bin)
    int r_n;
};

// idx = -0.5 + 0.5 sqrt(1 + 8 (d - lo) / bin) as the reference's float32 tensor ops round it: one subtraction, an exact scaling,
// one correctly rounded division, one addition, one correctly rounded square root; truncated toward zero; n where idx < 0,
// idx > n or idx is not finite.  sqrtf, NOT __fsqrt_rn: with this toolchain the latter is a bare v_sqrt_f32 (1 ulp) between two
// v_ldexp_f32, the former v_sqrt_f32 plus the two fma residual tests against its neighbours -- the correctly rounded root.
__device__ __forceinline__ int ld_depth_bin(float d, const LdBins &g)
{
#pragma clang fp contract(off)
    const float q = __fdiv_rn(8.f * __fsub_rn(d, g.d_lo), g.d_bin);
    const float idx = -0.5f + 0.5f * sqrtf(__fadd_rn(1.f, q));
    if (!(idx >= 0.f) || idx > (float)g.d_n || !(fabsf(idx) < INFINITY))
        return g.d_n;
    return (int)idx;
}

// r = (m - (lo - bin)) / bin; class trunc(r) - 1 for -1 <= r < n + 1, never below -1; -1 (no class) elsewhere and for NaN.
__device__ __forceinline__ int ld_rcs_class(float m, const LdBins &g)
{
#pragma clang fp contract(off)
    const float r = __fdiv_rn(__fsub_rn(m, g.r_off), g.r_bin);
    if (!(r >= -1.f) || !(r < (float)(g.r_n + 1)))
        return -1;
    return max((int)r - 1, -1);
}

// One workgroup per (image, feature row, column tile): ds map rows of ld_tile(ds) columns -- whole blocks: the largest multiple of ds
// up to 256, one block where ds >= 256.  Pass 1: a thread per column, the column's min / max over the ds rows (lanes read adjacent addresses, the rows'
// loads are independent) into LDS.  Pass 2: a thread per feature pixel over its ds columns.  A NaN wins both the min and the max
// (torch.min / torch.max propagate it).
__host__ __device__ static inline int ld_tile(int ds) { return ds >= 256 ? ds : (256 / ds) * ds; }

__global__ __launch_bounds__(256) void ld_pool_kernel(const float *__restrict__ depth, const float *__restrict__ rcs, int H, int W, int ds,
                                                      int tiles, const LdBins g, float *__restrict__ pooled, int32_t *__restrict__ bins,
                                                      int32_t *__restrict__ rcs_class)
{
    __shared__ float s_min[LD_MAX_DS], s_max[LD_MAX_DS];
    const int h = H / ds, w = W / ds, tw = ld_tile(ds);
    const int tile = blockIdx.x % tiles, row = blockIdx.x / tiles;
    const int bn = row / h, i = row % h;
    const int c0 = tile * tw, c1 = min(c0 + tw, W);
    const size_t row0 = ((size_t)bn * H + (size_t)i * ds) * W;
    for (int c = c0 + threadIdx.x; c < c1; c += 256) {
        if (depth) {
            float m = LD_EMPTY_DEPTH;
#pragma unroll 8
            for (int r = 0; r < ds; ++r) {
                float v = depth[row0 + (size_t)r * W + c];
                v = v == 0.f ? LD_EMPTY_DEPTH : v;
                m = (v < m || v != v) ? v : m;
            }
            s_min[c - c0] = m;
        }
        if (rcs) {
            float m = LD_EMPTY_RCS;
#pragma unroll 8
            for (int r = 0; r < ds; ++r) {
                float v = rcs[row0 + (size_t)r * W + c];
                v = v < g.r_lo ? LD_EMPTY_RCS : v;
                m = (v > m || v != v) ? v : m;
            }
            s_max[c - c0] = m;
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < (c1 - c0) / ds; j += 256) {
        const size_t o = ((size_t)bn * h + i) * w + c0 / ds + j;
        if (depth) {
            float m = s_min[j * ds];
            for (int k = 1; k < ds; ++k) {
                const float v = s_min[j * ds + k];
                m = (v < m || v != v) ? v : m;
            }
            pooled[o] = m;
            bins[o] = ld_depth_bin(m, g);
        }
        if (rcs) {
            float m = s_max[j * ds];
            for (int k = 1; k < ds; ++k) {
                const float v = s_max[j * ds + k];
                m = (v > m || v != v) ? v : m;
            }
            rcs_class[o] = ld_rcs_class(m, g);
        }
    }
}

// A thread per output element [BN][D + 1 + E][hw]; lanes run over adjacent pixels.
__global__ __launch_bounds__(256) void ld_prior_kernel(const int32_t *__restrict__ bins, const int32_t *__restrict__ rcs_class,
                                                       const float *__restrict__ weight, const float *__restrict__ bias, int hw, int D,
                                                       int E, int n_rcs, long total, float *__restrict__ out)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total)
        return;
    const int CH = D + 1 + E;
    const int q = (int)(t % hw), ch = (int)((t / hw) % CH);
    const long pix = t / ((long)hw * CH) * hw + q;
    float v;
    if (ch <= D) {
        v = bins[pix] == ch ? 1.f : 0.f;
    } else {
        const int e = ch - D - 1, cls = rcs_class[pix];
        v = bias[e];
        if (cls >= 0 && cls < n_rcs)
            v = weight[(size_t)e * n_rcs + cls] + v;
    }
    out[t] = v;
}

// Stage 1: one workgroup per (embedding channel e, pixel segment), four waves; a wave owns a contiguous quarter of the segment and
// walks it in ascending order, 64 (class, gradient) pairs at a time: each lane loads one pair, the pairs are broadcast from the
// registers (v_readlane) and lane l adds the gradient to its class sums l, l + 64, ... (LD_MAX_GROUPS of them) where the class
// matches; every lane also sums the pixels without a class.  The bias gradient of a wave is the sum of its class sums (a lane's
// four, then a butterfly over the lanes) plus the classless pixels' -- short sums of sums, not one run over every pixel.  The four
// waves are added in ascending order and the segment's n_rcs + 1 sums stored; stage 2 adds the segments in ascending order.
#define LD_MAX_GROUPS 4
#define LD_SLOTS (64 * LD_MAX_GROUPS + 1)
__global__ __launch_bounds__(256) void ld_prior_bwd_kernel(const float *__restrict__ grad, const int32_t *__restrict__ rcs_class, int BN,
                                                           int hw, int D, int E, int n_rcs, int segs, float *__restrict__ part)
{
    __shared__ float s_sum[4][LD_SLOTS];
    const int e = blockIdx.x / segs, seg = blockIdx.x % segs, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long M = (long)BN * hw, per = (M + segs * 4 - 1) / (segs * 4);
    const long p0 = min((seg * 4 + wave) * per, M), p1 = min(p0 + per, M);
    const int CH = D + 1 + E, groups = (n_rcs + 63) >> 6;
    float acc[LD_MAX_GROUPS], all = 0.f;
#pragma unroll
    for (int k = 0; k < LD_MAX_GROUPS; ++k)
        acc[k] = 0.f;
    for (long base = p0; base < p1; base += 64) {
        const long p = base + lane;
        int cls = -1;
        float gv = 0.f;                                     // (a lane past the end holds "no class, 0": it adds nothing)
        if (p < p1) {
            cls = rcs_class[p];
            gv = grad[((p / hw) * CH + D + 1 + e) * hw + p % hw];
        }
#pragma unroll
        for (int i = 0; i < 64; ++i) {
            const int raw = __builtin_amdgcn_readlane(cls, i), c = raw < n_rcs ? raw : -1;   // (a class >= n_rcs: the bias alone, as forward)
            const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gv), i));
            all += c < 0 ? v : 0.f;
#pragma unroll
            for (int k = 0; k < LD_MAX_GROUPS; ++k)
                if (k < groups)
                    acc[k] += c == lane + 64 * k ? v : 0.f;
        }
    }
#pragma unroll
    for (int k = 0; k < LD_MAX_GROUPS; ++k)
        s_sum[wave][lane + 64 * k] = acc[k];
    float tot = (acc[0] + acc[1]) + (acc[2] + acc[3]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        tot += __shfl_xor(tot, o);
    if (lane == 0)
        s_sum[wave][64 * LD_MAX_GROUPS] = tot + all;
    __syncthreads();
    for (int c = threadIdx.x; c <= n_rcs; c += 256) {
        const int slot = c < n_rcs ? c : 64 * LD_MAX_GROUPS;
        part[((size_t)seg * E + e) * (n_rcs + 1) + c] = ((s_sum[0][slot] + s_sum[1][slot]) + s_sum[2][slot]) + s_sum[3][slot];
    }
}

// Stage 2: a thread per (e, class or bias): the segments' sums in ascending order.
__global__ __launch_bounds__(256) void ld_prior_bwd_finish_kernel(const float *__restrict__ part, int E, int n_rcs, int segs,
                                                                  float *__restrict__ grad_weight, float *__restrict__ grad_bias)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= E * (n_rcs + 1))
        return;
    float s = part[t];
    for (int k = 1; k < segs; ++k)
        s += part[(size_t)k * E * (n_rcs + 1) + t];
    const int e = t / (n_rcs + 1), c = t % (n_rcs + 1);
    if (c < n_rcs)
        grad_weight[(size_t)e * n_rcs + c] = s;
    else
        grad_bias[e] = s;
}

// 64 pixels per workgroup, a lane per pixel (adjacent lanes read adjacent addresses of every channel plane); the D channels are cut
// into LD_LOSS_G contiguous runs, one wave each, and the runs' maxima and sums meet in LDS in run order -- the f8 problem is 66
// workgroups of 8 waves, 12 channels a wave.  Per foreground pixel (label < D), with t_c = onehot_c + 1e-6 (the reference's
// one_hot(eps = 1e-6)):
//   l      = sum_c t_c (-alpha) (1 - p_c)^2 log p_c                          p = softmax, log p = log-softmax
//   h_c    = t_c (-alpha) ((1 - p_c)^2 - 2 (1 - p_c) p_c log p_c)            = dl / d(log p_c)
//   grad_j = h_j - p_j sum_c h_c
// Background pixels write zeros.  partial[wg] = (sum of l over the 64 pixels, foreground count); pixel_loss (or NULL) = l.
#define LD_LOSS_G 8
__device__ __forceinline__ float ld_sum8(const float (*s)[64], int lane)
{
    return ((s[0][lane] + s[1][lane]) + (s[2][lane] + s[3][lane])) + ((s[4][lane] + s[5][lane]) + (s[6][lane] + s[7][lane]));
}

__global__ __launch_bounds__(64 * LD_LOSS_G) void ld_loss_kernel(const float *__restrict__ logits, const int32_t *__restrict__ labels, long M,
                                                                  int D, int hw, float alpha, float *__restrict__ partial,
                                                                  float *__restrict__ grad, float *__restrict__ pixel_loss)
{
#pragma clang fp contract(off)
    __shared__ float s_a[LD_LOSS_G][64], s_b[LD_LOSS_G][64], s_l[64], s_h[64];
    const int lane = threadIdx.x & 63, run = threadIdx.x >> 6;
    const long p = (long)blockIdx.x * 64 + lane;
    const bool live = p < M;
    const int label = live ? labels[p] : D;
    const bool fg = live && label >= 0 && label < D;
    const size_t base = live ? ((size_t)(p / hw) * D) * hw + p % hw : 0;
    const int per = (D + LD_LOSS_G - 1) / LD_LOSS_G, ca = min(run * per, D), cb = min(ca + per, D);
    const float *x = logits + base;
    float *g = grad + base;
    // (every barrier below is reached by all threads: the foreground test only guards the arithmetic)
    float mx = -INFINITY;
    if (fg)
        for (int c = ca; c < cb; ++c)
            mx = fmaxf(mx, x[(size_t)c * hw]);
    s_a[run][lane] = mx;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < LD_LOSS_G; ++r)
        mx = fmaxf(mx, s_a[r][lane]);
    float sum = 0.f;
    if (fg)
        for (int c = ca; c < cb; ++c)
            sum += expf(x[(size_t)c * hw] - mx);
    s_b[run][lane] = sum;
    __syncthreads();
    sum = ld_sum8(s_b, lane);
    const float lse = fg ? logf(sum) : 0.f;
    // the label's term is a million times the others: those are summed among themselves and the label's is added last (added in
    // channel order, the small terms behind it would each be rounded at the large one's scale)
    float lrest = 0.f, hrest = 0.f;
    if (fg)
        for (int c = ca; c < cb; ++c) {
            const float z = x[(size_t)c * hw] - mx;
            const float pc = __fdiv_rn(expf(z), sum), lp = z - lse;
            const float t = c == label ? 1.f + 1e-6f : 1e-6f;
            const float om = 1.f - pc;
            const float lc = t * (-alpha * (om * om) * lp), hc = t * -alpha * (om * om - 2.f * om * pc * lp);
            lrest += c == label ? 0.f : lc;
            hrest += c == label ? 0.f : hc;
            if (c == label) {
                s_l[lane] = lc;
                s_h[lane] = hc;
            }
        }
    __syncthreads();                                   // (s_a, s_b: every thread has read its maxima and sums)
    s_a[run][lane] = lrest;
    s_b[run][lane] = hrest;
    __syncthreads();
    const float loss = fg ? ld_sum8(s_a, lane) + s_l[lane] : 0.f;
    const float hsum = fg ? ld_sum8(s_b, lane) + s_h[lane] : 0.f;
    if (fg) {
        for (int c = ca; c < cb; ++c) {
            const float z = x[(size_t)c * hw] - mx;
            const float pc = __fdiv_rn(expf(z), sum), lp = z - lse;
            const float t = c == label ? 1.f + 1e-6f : 1e-6f;
            const float om = 1.f - pc;
            g[(size_t)c * hw] = t * -alpha * (om * om - 2.f * om * pc * lp) - pc * hsum;
        }
    } else if (live) {
        for (int c = ca; c < cb; ++c)
            g[(size_t)c * hw] = 0.f;
    }
    if (run != 0)
        return;
    if (pixel_loss && live)
        pixel_loss[p] = loss;
    const int count = __popcll(__ballot(fg));
    float total = loss;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        total += __shfl_xor(total, o);
    if (lane == 0) {
        partial[2 * (size_t)blockIdx.x] = total;
        partial[2 * (size_t)blockIdx.x + 1] = (float)count;      // (<= 64: exact)
    }
}

// One wave: lane l adds its contiguous run of pairs in index order, lane 0 then the 64 runs in lane order.
__global__ __launch_bounds__(64) void ld_loss_finish_kernel(const float *__restrict__ partial, int n, float weight, float *__restrict__ loss,
                                                            float *__restrict__ scale)
{
    __shared__ float s_sum[64];
    __shared__ int s_cnt[64];
    const int per = (n + 63) / 64, i0 = min((int)threadIdx.x * per, n), i1 = min(i0 + per, n);
    float s = 0.f;
    int cnt = 0;
    for (int i = i0; i < i1; ++i) {
        s += partial[2 * (size_t)i];
        cnt += (int)partial[2 * (size_t)i + 1];
    }
    s_sum[threadIdx.x] = s;
    s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int l = 1; l < 64; ++l) {
            s += s_sum[l];
            cnt += s_cnt[l];
        }
        const float denom = fmaxf(1.f, (float)cnt);
        *loss = __fdiv_rn(weight * s, denom);
        *scale = __fdiv_rn(weight, denom);
    }
}

__global__ __launch_bounds__(256) void ld_loss_bwd_kernel(const float *__restrict__ unit, const float *__restrict__ scale,
                                                          const float *__restrict__ grad_loss, long n, float *__restrict__ out)
{
    const float f = *scale * *grad_loss;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        out[i] = unit[i] * f;
}

extern "C" int rac_lss_pool_bins_fwd(const float *depth, const float *rcs, float *pooled, int32_t *bins, int32_t *rcs_class, int BN, int H,
                                     int W, int ds, float depth_lo, float depth_bin_size, int depth_bins, float rcs_lo, float rcs_offset,
                                     float rcs_bin_size, int rcs_bins, void *stream)
{
    RAC_CHECK_ARG(BN >= 0 && H > 0 && W > 0 && ds >= 1, "rac_lss_pool_bins_fwd: BN=%d H=%d W=%d ds=%d", BN, H, W, ds);
    RAC_CHECK_ARG(H % ds == 0 && W % ds == 0, "rac_lss_pool_bins_fwd: %d x %d map is not a multiple of ds=%d", H, W, ds);
    RAC_CHECK_ARG(depth || rcs, "rac_lss_pool_bins_fwd: null pointer (neither a depth nor an RCS map)");
    RAC_CHECK_ARG(!depth || (pooled && bins), "rac_lss_pool_bins_fwd: null pointer (pooled / bins of the depth map)");
    RAC_CHECK_ARG(!rcs || rcs_class, "rac_lss_pool_bins_fwd: null pointer (rcs_class of the RCS map)");
    RAC_CHECK_ARG(!depth || (depth_bins >= 1 && depth_bin_size > 0.f), "rac_lss_pool_bins_fwd: depth_bins=%d depth_bin_size=%g", depth_bins,
                  depth_bin_size);
    RAC_CHECK_ARG(!rcs || (rcs_bins >= 1 && rcs_bin_size > 0.f), "rac_lss_pool_bins_fwd: rcs_bins=%d rcs_bin_size=%g", rcs_bins, rcs_bin_size);
    if (ds > LD_MAX_DS) {
        rac_set_error("rac_lss_pool_bins_fwd: ds=%d exceeds %d", ds, LD_MAX_DS);
        return RAC_E_UNSUPPORTED;
    }
    const int tiles = (W + ld_tile(ds) - 1) / ld_tile(ds);
    RAC_CHECK_ARG((int64_t)BN * (H / ds) * tiles < ((int64_t)1 << 31), "rac_lss_pool_bins_fwd: %d maps of %d rows are too many", BN, H / ds);
    if (BN == 0)
        return 0;
    const LdBins g = {depth_lo, depth_bin_size, depth_bins, rcs_lo, rcs_offset, rcs_bin_size, rcs_bins};
    hipLaunchKernelGGL(ld_pool_kernel, dim3((unsigned)(BN * (H / ds) * tiles)), dim3(256), 0, (hipStream_t)stream, depth, rcs, H, W, ds, tiles, g,
                       pooled,
                       bins, rcs_class);
    return rac_launch_status("rac_lss_pool_bins_fwd");
}

static int ld_prior_args(const char *what, int BN, int hw, int D, int E, int n_rcs)
{
    RAC_CHECK_ARG(BN >= 0 && hw > 0, "%s: BN=%d hw=%d", what, BN, hw);
    RAC_CHECK_ARG(D >= 1 && E >= 1 && n_rcs >= 1, "%s: D=%d E=%d n_rcs=%d (all >= 1)", what, D, E, n_rcs);
    RAC_CHECK_ARG((int64_t)BN * hw * (D + 1 + E) < ((int64_t)1 << 40), "%s: %d x %d pixels x %d channels are too many", what, BN, hw, D + 1 + E);
    return 0;
}

extern "C" int rac_lss_prior_fwd(const int32_t *bins, const int32_t *rcs_class, const float *weight, const float *bias, float *out, int BN,
                                 int hw, int D, int E, int n_rcs, void *stream)
{
    if (int rc = ld_prior_args("rac_lss_prior_fwd", BN, hw, D, E, n_rcs))
        return rc;
    RAC_CHECK_ARG(bins && rcs_class && weight && bias && out, "rac_lss_prior_fwd: null pointer");
    if (BN == 0)
        return 0;
    const long total = (long)BN * hw * (D + 1 + E);
    hipLaunchKernelGGL(ld_prior_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bins, rcs_class, weight, bias,
                       hw, D, E, n_rcs, total, out);
    return rac_launch_status("rac_lss_prior_fwd");
}

extern "C" int rac_lss_prior_bwd(const float *grad_out, const int32_t *rcs_class, float *workspace, float *grad_weight, float *grad_bias,
                                 int BN, int hw, int D, int E, int n_rcs, void *stream)
{
    if (int rc = ld_prior_args("rac_lss_prior_bwd", BN, hw, D, E, n_rcs))
        return rc;
    RAC_CHECK_ARG(grad_out && rcs_class && workspace && grad_weight && grad_bias, "rac_lss_prior_bwd: null pointer");
    if (n_rcs > 64 * LD_MAX_GROUPS) {
        rac_set_error("rac_lss_prior_bwd: n_rcs=%d exceeds %d classes", n_rcs, 64 * LD_MAX_GROUPS);
        return RAC_E_UNSUPPORTED;
    }
    RAC_CHECK_ARG((int64_t)E * (n_rcs + 1) * LD_MAX_SEGS < ((int64_t)1 << 31), "rac_lss_prior_bwd: E=%d is too large", E);
    // 512 pixels a segment (128 a wave) where there are enough of them: the f8 problem is 32 x 8 workgroups
    const long M = (long)BN * hw;
    const int segs = (int)(M >= 512L * LD_MAX_SEGS ? LD_MAX_SEGS : (M + 511) / 512 > 0 ? (M + 511) / 512 : 1);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ld_prior_bwd_kernel, dim3((unsigned)(E * segs)), dim3(256), 0, st, grad_out, rcs_class, BN, hw, D, E, n_rcs, segs,
                       workspace);
    hipLaunchKernelGGL(ld_prior_bwd_finish_kernel, dim3((unsigned)((E * (n_rcs + 1) + 255) / 256)), dim3(256), 0, st, workspace, E, n_rcs,
                       segs, grad_weight, grad_bias);
    return rac_launch_status("rac_lss_prior_bwd");
}

extern "C" int rac_lss_depth_loss_fwd(const float *logits, const int32_t *labels, float *partial, float *grad_unit, float *pixel_loss, float *loss,
                                      float *scale, int BN, int D, int hw, float alpha, float gamma, float weight, void *stream)
{
    RAC_CHECK_ARG(BN >= 0 && hw > 0, "rac_lss_depth_loss_fwd: BN=%d hw=%d", BN, hw);
    RAC_CHECK_ARG(D >= 1, "rac_lss_depth_loss_fwd: D=%d (>= 1)", D);
    RAC_CHECK_ARG(partial && loss && scale && (BN == 0 || (logits && labels && grad_unit)), "rac_lss_depth_loss_fwd: null pointer");
    if (gamma != 2.f) {
        rac_set_error("rac_lss_depth_loss_fwd: built for gamma = 2, got %g", gamma);
        return RAC_E_UNSUPPORTED;
    }
    const long M = (long)BN * hw;
    RAC_CHECK_ARG(M < ((long)1 << 36), "rac_lss_depth_loss_fwd: %d x %d pixels are too many", BN, hw);
    const int n_wg = (int)((M + 63) / 64);
    hipStream_t st = (hipStream_t)stream;
    if (n_wg > 0)
        hipLaunchKernelGGL(ld_loss_kernel, dim3(n_wg), dim3(64 * LD_LOSS_G), 0, st, logits, labels, M, D, hw, alpha, partial, grad_unit, pixel_loss);
    hipLaunchKernelGGL(ld_loss_finish_kernel, dim3(1), dim3(64), 0, st, partial, n_wg, weight, loss, scale);
    return rac_launch_status("rac_lss_depth_loss_fwd");
}

extern "C" int rac_lss_depth_loss_bwd(const float *grad_unit, const float *scale, const float *grad_loss, float *grad_logits, int64_t n,
                                      void *stream)
{
    RAC_CHECK_ARG(n >= 0, "rac_lss_depth_loss_bwd: n=%lld", (long long)n);
    RAC_CHECK_ARG(scale && grad_loss && (n == 0 || (grad_unit && grad_logits)), "rac_lss_depth_loss_bwd: null pointer");
    if (n == 0)
        return 0;
    const long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(ld_loss_bwd_kernel, dim3((unsigned)(blocks > 2048 ? 2048 : blocks)), dim3(256), 0, (hipStream_t)stream, grad_unit, scale,
                       grad_loss, (long)n, grad_logits);
    return rac_launch_status("rac_lss_depth_loss_bwd");
}
