// optimizer.hip -- the training step's parameter update (gfx950): gradient norm, clip coefficient and AdamW over every trainable
// tensor in three launches (racformer_amd/optim.py, FusedAdamW.step).
//
// torch.optim.AdamW (amsgrad=False, maximize=False) after torch.nn.utils.clip_grad_norm_(norm_type=2), restated so that
//   * the norm is summed in an order this file fixes (no atomics, no dependence on the grid, the device or the addresses),
//   * nothing is read back (a non-finite norm skips the step on the device; step counters, bias corrections and the clip coefficient
//     live in device memory), so a step is capturable and a scheduler changes lr / weight decay by writing a device table,
//   * no library launch walks the parameter list.
//
// The unit of work is a CHUNK: RAC_OPT_CHUNK consecutive elements of ONE tensor (the last chunk of a tensor is short).  The host
// tables (rac_opt_tensor, rac_opt_chunk) say which.  Inside a chunk, lane t of the 256 owns elements 1024 * i + 4 * t + k (i < 16,
// k < 4) and visits them in (i, k) order, whether it gets them by one 16-byte access (base pointer 16-byte aligned and all four inside
// the tensor) or by four scalar ones -- the summation order does not depend on alignment.
//
//   1  opt_sumsq_kernel   one workgroup per chunk: the squares in float64 (a float32 square is exact there and FLT_MAX^2 fits), lane
//                         sums in the order above, a butterfly over the wave's lanes, the four waves through LDS in wave order ->
//                         partials[chunk]
//   2  opt_finish_kernel  one workgroup: lane t sums partials[t], partials[t + 256], ... in that order, then the same tree -> the
//                         record (sum of squares, norm, clip coefficient, skip).  Unless skipped: every present tensor's step counter
//                         + 1 and its scalars, computed in float64 from the hyper table's row and rounded once to float32
//   3  opt_update_kernel  one workgroup per chunk: returns without a store when skip is set; otherwise per element, every operation
//                         rounded once (no contraction), division and square root correctly rounded:
//                             g' = g * clip_coef;  p = p * (1 - lr wd);  m = m + (g' - m)(1 - b1);  v = b2 v + ((1 - b2) g') g'
//                             p = p - (lr / bc1) * (m / (sqrt(v) / sqrt(bc2) + eps))
// A non-finite gradient needs no flag: it makes the sum non-finite.
#include "rac_common.h"

#define OPT_THREADS 256
#define OPT_WAVES (OPT_THREADS / RAC_WAVE)
#define OPT_ITERS (RAC_OPT_CHUNK / (OPT_THREADS * 4))
static_assert(RAC_OPT_CHUNK % (OPT_THREADS * 4) == 0, "a chunk is a whole number of 16-byte passes of the workgroup");

// The tensors' pointers come out of a device table, so the compiler cannot tell their address space and would emit flat accesses; they
// are global memory by the entry's contract, and these casts say so (global_load / global_store).
#define OPT_GLOBAL __attribute__((address_space(1)))

// Four consecutive elements e .. e + 3 of a tensor of n (zeros past the end): one 16-byte load where `vec` (the base is 16-byte
// aligned; e is a multiple of 4) and all four exist.
__device__ __forceinline__ rac_f4 opt_ld4(const float *base, long e, long n, bool vec)
{
    const OPT_GLOBAL float *g = (const OPT_GLOBAL float *)base;
    if (vec && e + 4 <= n) {
        const rac_f4v v = *(const OPT_GLOBAL rac_f4v *)(g + e);
        return rac_f4{v.x, v.y, v.z, v.w};
    }
    rac_f4 o;
    o.x = e + 0 < n ? g[e + 0] : 0.f;
    o.y = e + 1 < n ? g[e + 1] : 0.f;
    o.z = e + 2 < n ? g[e + 2] : 0.f;
    o.w = e + 3 < n ? g[e + 3] : 0.f;
    return o;
}

__device__ __forceinline__ void opt_st4(float *base, long e, long n, bool vec, const rac_f4 v)
{
    OPT_GLOBAL float *g = (OPT_GLOBAL float *)base;
    if (vec && e + 4 <= n) {
        *(OPT_GLOBAL rac_f4v *)(g + e) = (rac_f4v){v.x, v.y, v.z, v.w};
        return;
    }
    if (e + 0 < n) g[e + 0] = v.x;
    if (e + 1 < n) g[e + 1] = v.y;
    if (e + 2 < n) g[e + 2] = v.z;
    if (e + 3 < n) g[e + 3] = v.w;
}

__device__ __forceinline__ bool opt_aligned16(const void *p)
{
    return (reinterpret_cast<uintptr_t>(p) & 15) == 0;
}

// The workgroup's sum of one double per lane, in a fixed tree: butterfly over the 64 lanes of a wave (every lane ends with the same
// bits: each level adds the same two values in either order), then wave 0 .. 3 in order.  Every lane returns the total.
__device__ __forceinline__ double opt_block_sum(double acc, double *lds)
{
#pragma unroll
    for (int off = RAC_WAVE / 2; off >= 1; off >>= 1)
        acc += __shfl_xor(acc, off, RAC_WAVE);
    if ((threadIdx.x & (RAC_WAVE - 1)) == 0)
        lds[threadIdx.x / RAC_WAVE] = acc;
    __syncthreads();
    double total = lds[0];
#pragma unroll
    for (int w = 1; w < OPT_WAVES; ++w)
        total += lds[w];
    return total;
}

__global__ __launch_bounds__(OPT_THREADS) void opt_sumsq_kernel(const rac_opt_tensor *__restrict__ tensors,
                                                                const rac_opt_chunk *__restrict__ chunks, double *__restrict__ partials)
{
    __shared__ double lds[OPT_WAVES];
    const rac_opt_chunk c = chunks[blockIdx.x];
    const rac_opt_tensor t = tensors[c.tensor];
    const float *__restrict__ g = t.g + c.start;
    const long n = t.numel - c.start < RAC_OPT_CHUNK ? t.numel - c.start : (long)RAC_OPT_CHUNK;
    const bool vec = opt_aligned16(g);
    double acc = 0.0;
#pragma unroll 4
    for (int i = 0; i < OPT_ITERS; ++i) {
        const long e = (long)i * (OPT_THREADS * 4) + threadIdx.x * 4;
        if (e < n) {
            const rac_f4 v = opt_ld4(g, e, n, vec);
            acc += (double)v.x * (double)v.x;
            acc += (double)v.y * (double)v.y;
            acc += (double)v.z * (double)v.z;
            acc += (double)v.w * (double)v.w;
        }
    }
    const double total = opt_block_sum(acc, lds);
    if (threadIdx.x == 0)
        partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(OPT_THREADS) void opt_finish_kernel(const rac_opt_tensor *__restrict__ tensors, int n_tensors,
                                                                 const double *__restrict__ partials, int n_chunks,
                                                                 const double *__restrict__ hyper, float *__restrict__ steps,
                                                                 float *__restrict__ scalars, rac_opt_record *__restrict__ record,
                                                                 float max_norm)
{
    __shared__ double lds[OPT_WAVES];
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_chunks; i += OPT_THREADS)
        acc += partials[i];
    const double total = opt_block_sum(acc, lds);
    const bool finite = total - total == 0.0;                   // (inf - inf and nan - nan are nan)
    const double norm = sqrt(total);
    double coef = 1.0;
    if (max_norm >= 0.f) {
        coef = (double)max_norm / (norm + 1e-6);
        coef = coef < 1.0 ? coef : 1.0;                         // (a nan stays out: the step is skipped then anyway)
    }
    if (threadIdx.x == 0) {
        record->total_sq = total;
        record->total_norm = norm;
        record->clip_coef = (float)coef;
        record->skip = finite ? 0 : 1;
    }
    if (!finite)
        return;
    for (int i = threadIdx.x; i < n_tensors; i += OPT_THREADS) {
        const int row = tensors[i].row;
        const double *__restrict__ h = hyper + (long)row * RAC_OPT_HYPER;
        const double lr = h[0], wd = h[1], b1 = h[2], b2 = h[3], eps = h[4];
        const float step = steps[row] + 1.f;
        steps[row] = step;
        const double bc1 = 1.0 - pow(b1, (double)step);
        const double bc2 = 1.0 - pow(b2, (double)step);
        float *__restrict__ s = scalars + (long)row * RAC_OPT_SCALARS;
        s[0] = (float)(1.0 - lr * wd);
        s[1] = (float)(lr / bc1);
        s[2] = (float)sqrt(bc2);
        s[3] = (float)(1.0 - b1);
        s[4] = (float)b2;
        s[5] = (float)(1.0 - b2);
        s[6] = (float)eps;
        s[7] = 0.f;
    }
}

struct opt_scalars {
    float clip, decay, step_size, sqrt_bc2, one_minus_b1, b2, one_minus_b2, eps;
};

// One element.  Every operation rounds once: no fused multiply-add is formed here, so the result is the formula's as written.
__device__ __forceinline__ void opt_update_one(float g, float &p, float &m, float &v, const opt_scalars &s)
{
#pragma clang fp contract(off)
    const float gc = g * s.clip;
    const float pd = p * s.decay;
    const float m1 = m + (gc - m) * s.one_minus_b1;
    const float v1 = s.b2 * v + (s.one_minus_b2 * gc) * gc;
    const float denom = sqrtf(v1) / s.sqrt_bc2 + s.eps;
    p = pd - s.step_size * (m1 / denom);
    m = m1;
    v = v1;
}

__global__ __launch_bounds__(OPT_THREADS) void opt_update_kernel(const rac_opt_tensor *__restrict__ tensors,
                                                                 const rac_opt_chunk *__restrict__ chunks,
                                                                 const float *__restrict__ scalars, const rac_opt_record *__restrict__ record)
{
    if (record->skip)
        return;
    const rac_opt_chunk c = chunks[blockIdx.x];
    const rac_opt_tensor t = tensors[c.tensor];
    const float *__restrict__ row = scalars + (long)t.row * RAC_OPT_SCALARS;
    const opt_scalars s = {record->clip_coef, row[0], row[1], row[2], row[3], row[4], row[5], row[6]};
    const float *__restrict__ g = t.g + c.start;
    float *__restrict__ p = t.p + c.start;
    float *__restrict__ m = t.m + c.start;
    float *__restrict__ v = t.v + c.start;
    const long n = t.numel - c.start < RAC_OPT_CHUNK ? t.numel - c.start : (long)RAC_OPT_CHUNK;
    const bool vg = opt_aligned16(g), vp = opt_aligned16(p), vm = opt_aligned16(m), vv = opt_aligned16(v);
#pragma unroll 2
    for (int i = 0; i < OPT_ITERS; ++i) {
        const long e = (long)i * (OPT_THREADS * 4) + threadIdx.x * 4;
        if (e < n) {
            const rac_f4 g4 = opt_ld4(g, e, n, vg);
            rac_f4 p4 = opt_ld4(p, e, n, vp), m4 = opt_ld4(m, e, n, vm), v4 = opt_ld4(v, e, n, vv);
            opt_update_one(g4.x, p4.x, m4.x, v4.x, s);
            opt_update_one(g4.y, p4.y, m4.y, v4.y, s);
            opt_update_one(g4.z, p4.z, m4.z, v4.z, s);
            opt_update_one(g4.w, p4.w, m4.w, v4.w, s);
            opt_st4(p, e, n, vp, p4);
            opt_st4(m, e, n, vm, m4);
            opt_st4(v, e, n, vv, v4);
        }
    }
}

extern "C" int rac_adamw_step(const rac_opt_tensor *tensors, int n_tensors, const rac_opt_chunk *chunks, int n_chunks,
                              const double *hyper, float *steps, float *scalars, double *partials, rac_opt_record *record,
                              float max_norm, int phases, void *stream)
{
    RAC_CHECK_ARG(tensors && chunks && hyper && steps && scalars && partials && record, "rac_adamw_step: null pointer");
    RAC_CHECK_ARG(n_tensors >= 1 && n_chunks >= n_tensors, "rac_adamw_step: n_tensors=%d n_chunks=%d (at least one chunk per tensor)",
                  n_tensors, n_chunks);
    RAC_CHECK_ARG(phases >= 1 && phases <= RAC_OPT_ALL, "rac_adamw_step: phases=%d (a mask of RAC_OPT_NORM | RAC_OPT_FINISH | RAC_OPT_UPDATE)",
                  phases);
    RAC_CHECK_ARG(max_norm == max_norm, "rac_adamw_step: max_norm is nan (negative: no clipping)");
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(tensors) | reinterpret_cast<uintptr_t>(chunks) | reinterpret_cast<uintptr_t>(hyper) |
                    reinterpret_cast<uintptr_t>(partials) | reinterpret_cast<uintptr_t>(record)) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(steps) | reinterpret_cast<uintptr_t>(scalars)) & 3) == 0,
                  "rac_adamw_step: misaligned table");
    hipStream_t s = (hipStream_t)stream;
    if (phases & RAC_OPT_NORM) {
        hipLaunchKernelGGL(opt_sumsq_kernel, dim3((unsigned)n_chunks), dim3(OPT_THREADS), 0, s, tensors, chunks, partials);
        if (int rc = rac_launch_status("rac_adamw_step (sum of squares)"))
            return rc;
    }
    if (phases & RAC_OPT_FINISH) {
        hipLaunchKernelGGL(opt_finish_kernel, dim3(1), dim3(OPT_THREADS), 0, s, tensors, n_tensors, partials, n_chunks, hyper, steps, scalars,
                           record, max_norm);
        if (int rc = rac_launch_status("rac_adamw_step (finish)"))
            return rc;
    }
    if (phases & RAC_OPT_UPDATE) {
        hipLaunchKernelGGL(opt_update_kernel, dim3((unsigned)n_chunks), dim3(OPT_THREADS), 0, s, tensors, chunks, scalars, record);
        if (int rc = rac_launch_status("rac_adamw_step (update)"))
            return rc;
    }
    return 0;
}
