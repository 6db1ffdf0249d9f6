// batchnorm_train.hip -- training-mode BatchNorm (+ ReLU) on channel-first fp32 maps [N][C][HW], forward and backward, gfx950: the
// BatchNorm2d of radar_bev_conv's ConvModules when the radar pillar branch trains (models/racformer.py:316-331 runs frame 0 in
// training mode under autograd), the first BatchNorm of the project that cannot be folded into its convolution.
//
// A channel's n = N * HW elements, in (image, pixel) order, are cut into chunks of BNT_CHUNK; one workgroup sums one chunk of one
// channel, a second launch adds the chunks in ascending order.  All sums are float64 (sum x and sum x^2: the squares of float32 values
// are exact in float64, so var = sum x^2 / n - mean^2 loses mean^2 / var * 2^-52 relative -- 2e-10 at |mean| = 1e3 std, where the
// same expression in float32 has no correct digit).  Inside a workgroup: a thread's elements in ascending order, the lanes by a
// butterfly (commutative pairs: every lane holds the same sum), the four waves in ascending order.  No atomics, geometry from the
// shapes alone, nothing read back: capturable, bitwise reproducible.
#include "rac_common.h"

#define BNT_THREADS 256
#define BNT_PER_THREAD 16
#define BNT_CHUNK (BNT_THREADS * BNT_PER_THREAD)
#define BNT_ROW_BLOCK 1024                   // elements of one (image, channel) row per workgroup of the element-wise kernels

__device__ __forceinline__ void bnt_block_sum2(double &a, double &b, double (*s)[4])
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o);
        b += __shfl_xor(b, o);
    }
    if ((threadIdx.x & 63) == 0) {
        s[0][threadIdx.x >> 6] = a;
        s[1][threadIdx.x >> 6] = b;
    }
    __syncthreads();
    a = ((s[0][0] + s[0][1]) + s[0][2]) + s[0][3];
    b = ((s[1][0] + s[1][1]) + s[1][2]) + s[1][3];
}

// part[c][k] = (sum x, sum x^2) over chunk k of channel c
__global__ __launch_bounds__(BNT_THREADS) void bnt_stats_part_kernel(const float *__restrict__ x, double *__restrict__ part, int C, int HW,
                                                                     long total, int K)
{
    __shared__ double s[2][4];
    const int c = blockIdx.y, k = blockIdx.x;
    double s1 = 0.0, s2 = 0.0;
    const long e0 = (long)k * BNT_CHUNK + threadIdx.x;
#pragma unroll 4
    for (int i = 0; i < BNT_PER_THREAD; ++i) {
        const long e = e0 + (long)i * BNT_THREADS;
        if (e < total) {
            const long n = e / HW;
            const double v = (double)x[(n * C + c) * HW + (e - n * HW)];
            s1 += v;
            s2 += v * v;
        }
    }
    bnt_block_sum2(s1, s2, s);
    if (threadIdx.x == 0) {
        part[((long)c * K + k) * 2 + 0] = s1;
        part[((long)c * K + k) * 2 + 1] = s2;
    }
}

// One thread per channel: the chunks in ascending order, then what nn.BatchNorm2d.forward updates in training mode.
__global__ __launch_bounds__(64) void bnt_stats_finish_kernel(const double *__restrict__ part, float *__restrict__ mean,
                                                              float *__restrict__ invstd, float *__restrict__ running_mean,
                                                              float *__restrict__ running_var, int64_t *__restrict__ tracked, int C, int K,
                                                              long total, float eps, float momentum)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C)
        return;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < K; ++k) {
        s1 += part[((long)c * K + k) * 2 + 0];
        s2 += part[((long)c * K + k) * 2 + 1];
    }
    const double n = (double)total, m = s1 / n;
    double var = s2 / n - m * m;
    var = var > 0.0 ? var : (var == var ? 0.0 : var);            // (a NaN stays)
    mean[c] = (float)m;
    invstd[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (running_mean) {
        const double mo = (double)momentum;
        running_mean[c] = (float)((1.0 - mo) * (double)running_mean[c] + mo * m);
        running_var[c] = (float)((1.0 - mo) * (double)running_var[c] + mo * (var * (n / (n - 1.0))));
        if (c == 0)
            *tracked += 1;
    }
}

// y = [relu]((x - mean) * invstd * gamma + beta), evaluated left to right in float32
__global__ __launch_bounds__(BNT_THREADS) void bnt_apply_kernel(const float *__restrict__ x, const float *__restrict__ mean,
                                                                const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, float *__restrict__ y, int C, int HW,
                                                                int row_blocks, int relu)
{
#pragma clang fp contract(off)
    const long row = blockIdx.x / row_blocks;
    const int p0 = (blockIdx.x % row_blocks) * BNT_ROW_BLOCK + threadIdx.x, c = (int)(row % C);
    const float m = mean[c], is = invstd[c], g = gamma[c], b = beta[c];
#pragma unroll
    for (int i = 0; i < BNT_ROW_BLOCK / BNT_THREADS; ++i) {
        const int p = p0 + i * BNT_THREADS;
        if (p < HW) {
            const float v = ((x[row * HW + p] - m) * is) * g + b;
            y[row * HW + p] = relu ? rac_relu(v) : v;
        }
    }
}

// part[c][k] = (sum gm, sum gm * xhat) over chunk k of channel c;  gm = g where y > 0 (y NULL: g as it is), xhat = (x - mean) * invstd
__global__ __launch_bounds__(BNT_THREADS) void bnt_bwd_part_kernel(const float *__restrict__ g, const float *__restrict__ x,
                                                                   const float *__restrict__ y, const float *__restrict__ mean,
                                                                   const float *__restrict__ invstd, double *__restrict__ part, int C,
                                                                   int HW, long total, int K)
{
#pragma clang fp contract(off)
    __shared__ double s[2][4];
    const int c = blockIdx.y, k = blockIdx.x;
    const float m = mean[c], is = invstd[c];
    double s1 = 0.0, s2 = 0.0;
    const long e0 = (long)k * BNT_CHUNK + threadIdx.x;
#pragma unroll 4
    for (int i = 0; i < BNT_PER_THREAD; ++i) {
        const long e = e0 + (long)i * BNT_THREADS;
        if (e < total) {
            const long n = e / HW, at = (n * C + c) * HW + (e - n * HW);
            const float gm = (!y || y[at] > 0.f) ? g[at] : 0.f;
            const float xh = (x[at] - m) * is;
            s1 += (double)gm;
            s2 += (double)gm * (double)xh;
        }
    }
    bnt_block_sum2(s1, s2, s);
    if (threadIdx.x == 0) {
        part[((long)c * K + k) * 2 + 0] = s1;
        part[((long)c * K + k) * 2 + 1] = s2;
    }
}

__global__ __launch_bounds__(64) void bnt_bwd_finish_kernel(const double *__restrict__ part, float *__restrict__ dgamma,
                                                            float *__restrict__ dbeta, int C, int K)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C)
        return;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < K; ++k) {
        s1 += part[((long)c * K + k) * 2 + 0];
        s2 += part[((long)c * K + k) * 2 + 1];
    }
    dbeta[c] = (float)s1;
    dgamma[c] = (float)s2;
}

// dx = gamma * invstd * (gm - dbeta / n - xhat * dgamma / n)
__global__ __launch_bounds__(BNT_THREADS) void bnt_bwd_dx_kernel(const float *__restrict__ g, const float *__restrict__ x,
                                                                 const float *__restrict__ y, const float *__restrict__ mean,
                                                                 const float *__restrict__ invstd, const float *__restrict__ gamma,
                                                                 const float *__restrict__ dgamma, const float *__restrict__ dbeta,
                                                                 float *__restrict__ dx, int C, int HW, int row_blocks, float inv_n)
{
#pragma clang fp contract(off)
    const long row = blockIdx.x / row_blocks;
    const int p0 = (blockIdx.x % row_blocks) * BNT_ROW_BLOCK + threadIdx.x, c = (int)(row % C);
    const float m = mean[c], is = invstd[c], k = gamma[c] * is, a = dbeta[c] * inv_n, b = dgamma[c] * inv_n;
#pragma unroll
    for (int i = 0; i < BNT_ROW_BLOCK / BNT_THREADS; ++i) {
        const int p = p0 + i * BNT_THREADS;
        if (p < HW) {
            const long at = row * HW + p;
            const float gm = (!y || y[at] > 0.f) ? g[at] : 0.f;
            const float xh = (x[at] - m) * is;
            dx[at] = k * ((gm - a) - xh * b);
        }
    }
}

static int bnt_check_shape(const char *what, int N, int C, int HW)
{
    RAC_CHECK_ARG(N >= 1 && HW >= 1 && C >= 64 && C <= 4096 && C % 64 == 0, "%s: N=%d C=%d HW=%d (C a multiple of 64, at most 4096)", what, N,
                  C, HW);
    RAC_CHECK_ARG((int64_t)N * HW >= 2, "%s: N * H * W = %lld: batch statistics need at least 2 values per channel", what,
                  (long long)N * HW);
    RAC_CHECK_ARG((int64_t)N * C * ((HW + BNT_ROW_BLOCK - 1) / BNT_ROW_BLOCK) < ((int64_t)1 << 31) &&
                      ((int64_t)N * HW + BNT_CHUNK - 1) / BNT_CHUNK < ((int64_t)1 << 31),
                  "%s: N=%d C=%d HW=%d is too large", what, N, C, HW);
    return 0;
}

static int bnt_chunks(int N, int HW) { return (int)(((int64_t)N * HW + BNT_CHUNK - 1) / BNT_CHUNK); }

extern "C" int rac_bn_train_stats_fwd(const float *x, double *workspace, float *mean, float *invstd, float *running_mean,
                                      float *running_var, int64_t *num_batches_tracked, int N, int C, int HW, float eps, float momentum,
                                      void *stream)
{
    if (int rc = bnt_check_shape("rac_bn_train_stats_fwd", N, C, HW))
        return rc;
    RAC_CHECK_ARG(x && workspace && mean && invstd, "rac_bn_train_stats_fwd: null pointer");
    RAC_CHECK_ARG((running_mean && running_var && num_batches_tracked) || (!running_mean && !running_var && !num_batches_tracked),
                  "rac_bn_train_stats_fwd: running_mean, running_var and num_batches_tracked are given together or not at all");
    RAC_CHECK_ARG(eps >= 0.f && momentum >= 0.f && momentum <= 1.f, "rac_bn_train_stats_fwd: eps=%g momentum=%g", eps, momentum);
    hipStream_t st = (hipStream_t)stream;
    const int K = bnt_chunks(N, HW);
    const long total = (long)N * HW;
    hipLaunchKernelGGL(bnt_stats_part_kernel, dim3(K, C), dim3(BNT_THREADS), 0, st, x, workspace, C, HW, total, K);
    hipLaunchKernelGGL(bnt_stats_finish_kernel, dim3(C / 64), dim3(64), 0, st, workspace, mean, invstd, running_mean, running_var,
                       num_batches_tracked, C, K, total, eps, momentum);
    return rac_launch_status("rac_bn_train_stats_fwd");
}

extern "C" int rac_bn_train_apply_fwd(const float *x, const float *mean, const float *invstd, const float *gamma, const float *beta,
                                      float *y, int N, int C, int HW, int relu, void *stream)
{
    if (int rc = bnt_check_shape("rac_bn_train_apply_fwd", N, C, HW))
        return rc;
    RAC_CHECK_ARG(x && mean && invstd && gamma && beta && y, "rac_bn_train_apply_fwd: null pointer");
    const int row_blocks = (HW + BNT_ROW_BLOCK - 1) / BNT_ROW_BLOCK;
    hipLaunchKernelGGL(bnt_apply_kernel, dim3((unsigned)((long)N * C * row_blocks)), dim3(BNT_THREADS), 0, (hipStream_t)stream, x, mean,
                       invstd, gamma, beta, y, C, HW, row_blocks, relu);
    return rac_launch_status("rac_bn_train_apply_fwd");
}

extern "C" int rac_bn_train_bwd(const float *g, const float *x, const float *y, const float *mean, const float *invstd,
                                const float *gamma, double *workspace, float *dgamma, float *dbeta, float *dx, int N, int C, int HW,
                                void *stream)
{
    if (int rc = bnt_check_shape("rac_bn_train_bwd", N, C, HW))
        return rc;
    RAC_CHECK_ARG(g && x && mean && invstd && gamma && workspace && dgamma && dbeta, "rac_bn_train_bwd: null pointer");
    RAC_CHECK_ARG(!dx || (dx != g && dx != x && dx != y), "rac_bn_train_bwd: dx must not alias an input");
    hipStream_t st = (hipStream_t)stream;
    const int K = bnt_chunks(N, HW);
    const long total = (long)N * HW;
    hipLaunchKernelGGL(bnt_bwd_part_kernel, dim3(K, C), dim3(BNT_THREADS), 0, st, g, x, y, mean, invstd, workspace, C, HW, total, K);
    hipLaunchKernelGGL(bnt_bwd_finish_kernel, dim3(C / 64), dim3(64), 0, st, workspace, dgamma, dbeta, C, K);
    if (dx) {
        const int row_blocks = (HW + BNT_ROW_BLOCK - 1) / BNT_ROW_BLOCK;
        hipLaunchKernelGGL(bnt_bwd_dx_kernel, dim3((unsigned)((long)N * C * row_blocks)), dim3(BNT_THREADS), 0, st, g, x, y, mean, invstd,
                           gamma, dgamma, dbeta, dx, C, HW, row_blocks, (float)(1.0 / (double)total));
    }
    return rac_launch_status("rac_bn_train_bwd");
}
