// refine.hip -- box refinement tail of a decoder layer as one kernel (gfx950).
//
// Replaces ~27 elementwise launches per layer: refine_bbox (models/racformer_transformer.py:230-236:
// theta += (2*sigmoid(d0)-1)/num_ray; (d,z) = sigmoid(delta + inverse_sigmoid(d,z)); dims 3..9 from the
// regression output), the velocity scaling by time_diff[:,1] (:265-269, values < 1e-5 replaced by 1) and
// the polar -> normalised-xy conversion of the emitted boxes (theta_d2xy_coods, models/bbox/utils.py:82-90;
// :134).  One thread per query; pure elementwise fp32.
#include "rac_common.h"

#define REF_TWO_PI 6.283185307179586f

__device__ __forceinline__ float ref_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ float ref_inverse_sigmoid(float x)
{
    // models/utils.py:86-101, eps = 1e-5
    x = fminf(fmaxf(x, 0.f), 1.f);
    const float x1 = fmaxf(x, 1e-5f), x2 = fmaxf(1.f - x, 1e-5f);
    return logf(x1 / x2);
}

__global__ __launch_bounds__(256) void refine_kernel(const float *__restrict__ prop, const float *__restrict__ delta,
                                                     const float *__restrict__ td_safe, float *__restrict__ pred,
                                                     float *__restrict__ xy, int n, int Q, int T, float num_ray)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const float *p = prop + (size_t)i * 10, *d = delta + (size_t)i * 10;
    float o[10];
    o[0] = p[0] + (ref_sigmoid(d[0]) * 2.f - 1.f) / num_ray;
    o[1] = ref_sigmoid(d[1] + ref_inverse_sigmoid(p[1]));
    o[2] = ref_sigmoid(d[2] + ref_inverse_sigmoid(p[2]));
#pragma unroll
    for (int k = 3; k < 10; ++k)
        o[k] = d[k];
    if (T > 1) {
        const float td = td_safe[(i / Q) * T + 1];
        o[8] = o[8] / td;
        o[9] = o[9] / td;
    }
    float *pp = pred + (size_t)i * 10, *px = xy + (size_t)i * 10;
#pragma unroll
    for (int k = 0; k < 10; ++k)
        pp[k] = o[k];
    const float ang = o[0] * REF_TWO_PI, rad = o[1] * 65.0f;
    px[0] = fminf(fmaxf((51.2f + rad * cosf(ang)) / 102.4f, 0.f), 1.f);
    px[1] = fminf(fmaxf((51.2f + rad * sinf(ang)) / 102.4f, 0.f), 1.f);
#pragma unroll
    for (int k = 2; k < 10; ++k)
        px[k] = o[k];
}

extern "C" int rac_refine_fwd(const float *proposal, const float *delta, const float *time_diff_safe, float *bbox_pred,
                              float *bbox_xy, int B, int Q, int T, float num_ray, void *stream)
{
    RAC_CHECK_ARG(B >= 0 && Q >= 0 && T >= 1 && num_ray > 0.f, "rac_refine_fwd: bad sizes B=%d Q=%d T=%d", B, Q, T);
    if (B * Q == 0)
        return 0;
    RAC_CHECK_ARG(proposal && delta && time_diff_safe && bbox_pred && bbox_xy, "rac_refine_fwd: null pointer");
    const int n = B * Q;
    hipLaunchKernelGGL(refine_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, proposal, delta,
                       time_diff_safe, bbox_pred, bbox_xy, n, Q, T, num_ray);
    return rac_launch_status("rac_refine_fwd");
}

// ------------------------------------------------------------------------------------------------ backward
// Closed-form backward of refine_kernel: (grad_pred, grad_xy) -> (grad_delta, grad_proposal), one thread per query, the forward
// quantities recomputed from proposal, delta and time_diff_safe.  The gates are torch's for the ops the reference uses: clamp
// passes the gradient on the closed interval and blocks it outside (the [0,1] clamp of theta_d2xy_coods on the value the forward
// kernel computes, the [0,1] clamp of inverse_sigmoid), and inverse_sigmoid's clamp(min=eps) of x and of 1-x each gate their
// own factor of d log(x1/x2) = dx1/x1 - dx2/x2.  A null grad_pred or grad_xy is skipped, not read.
__device__ __forceinline__ float ref_inverse_sigmoid_grad(float x)
{
    if (!(x >= 0.f && x <= 1.f))
        return 0.f;
    const float y = 1.f - x;
    return (x >= 1e-5f ? 1.f / x : 0.f) + (y >= 1e-5f ? 1.f / y : 0.f);
}

__global__ __launch_bounds__(256) void refine_bwd_kernel(const float *__restrict__ prop, const float *__restrict__ delta,
                                                         const float *__restrict__ td_safe, const float *__restrict__ gpred,
                                                         const float *__restrict__ gxy, float *__restrict__ gdelta,
                                                         float *__restrict__ gprop, int n, int Q, int T, float num_ray)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const float *p = prop + (size_t)i * 10, *d = delta + (size_t)i * 10;
    float go[10];
#pragma unroll
    for (int k = 0; k < 10; ++k)
        go[k] = gpred ? gpred[(size_t)i * 10 + k] : 0.f;
    const float s0 = ref_sigmoid(d[0]);
    const float o1 = ref_sigmoid(d[1] + ref_inverse_sigmoid(p[1]));
    const float o2 = ref_sigmoid(d[2] + ref_inverse_sigmoid(p[2]));
    if (gxy) {
        const float *gx = gxy + (size_t)i * 10;
        const float o0 = p[0] + (s0 * 2.f - 1.f) / num_ray;
        const float ang = o0 * REF_TWO_PI, rad = o1 * 65.0f;
        const float cs = cosf(ang), sn = sinf(ang);
        const float ux = (51.2f + rad * cs) / 102.4f, uy = (51.2f + rad * sn) / 102.4f;
        const float gux = (ux >= 0.f && ux <= 1.f) ? gx[0] / 102.4f : 0.f;
        const float guy = (uy >= 0.f && uy <= 1.f) ? gx[1] / 102.4f : 0.f;
        go[0] += (guy * cs - gux * sn) * rad * REF_TWO_PI;
        go[1] += (gux * cs + guy * sn) * 65.0f;
#pragma unroll
        for (int k = 2; k < 10; ++k)
            go[k] += gx[k];
    }
    float gd[10], gp[10];
    gd[0] = go[0] * (2.f * s0 * (1.f - s0) / num_ray);
    gp[0] = go[0];
    const float gs1 = go[1] * (o1 * (1.f - o1)), gs2 = go[2] * (o2 * (1.f - o2));
    gd[1] = gs1;
    gd[2] = gs2;
    gp[1] = gs1 * ref_inverse_sigmoid_grad(p[1]);
    gp[2] = gs2 * ref_inverse_sigmoid_grad(p[2]);
#pragma unroll
    for (int k = 3; k < 10; ++k) {
        gd[k] = go[k];
        gp[k] = 0.f;
    }
    if (T > 1) {
        const float td = td_safe[(i / Q) * T + 1];
        gd[8] = go[8] / td;
        gd[9] = go[9] / td;
    }
    float *pd = gdelta + (size_t)i * 10, *pp = gprop + (size_t)i * 10;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        pd[k] = gd[k];
        pp[k] = gp[k];
    }
}

extern "C" int rac_refine_bwd(const float *proposal, const float *delta, const float *time_diff_safe, const float *grad_pred,
                              const float *grad_xy, float *grad_delta, float *grad_proposal, int B, int Q, int T, float num_ray,
                              void *stream)
{
    RAC_CHECK_ARG(B >= 0 && Q >= 0 && T >= 1 && num_ray > 0.f, "rac_refine_bwd: bad sizes B=%d Q=%d T=%d", B, Q, T);
    if (B * Q == 0)
        return 0;
    RAC_CHECK_ARG(proposal && delta && time_diff_safe && grad_delta && grad_proposal, "rac_refine_bwd: null pointer");
    const int n = B * Q;
    hipLaunchKernelGGL(refine_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, proposal, delta, time_diff_safe,
                       grad_pred, grad_xy, grad_delta, grad_proposal, n, Q, T, num_ray);
    return rac_launch_status("rac_refine_bwd");
}

// ------------------------------------------------------------------------------------------------ head outputs
// What RaCFormerTransformer.forward and RaCFormer_head.forward do to the stacked decoder outputs, one launch instead of five:
//   cls  <- nan_to_num(cls)                                      (racformer_transformer.py:58)
//   box  <- nan_to_num(xy), then centre * pc_range span + origin and the (x, y, w, l, z, h, ...) column order
//           (racformer_head.py:124-131).  nan_to_num first, as the reference: a NaN centre becomes the range origin.
__device__ __forceinline__ float hf_nan_to_num(float v)
{
    if (v != v)
        return 0.f;
    return fminf(fmaxf(v, -3.4028234663852886e38f), 3.4028234663852886e38f);   // +-inf -> +-FLT_MAX (torch.nan_to_num defaults)
}

__global__ __launch_bounds__(256) void head_finish_kernel(float *__restrict__ cls, long n_cls, const float *__restrict__ xy,
                                                          float *__restrict__ box, long rows, float x0, float y0, float z0,
                                                          float sx, float sy, float sz)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_cls)
        cls[i] = hf_nan_to_num(cls[i]);
    if (i < rows) {
#pragma clang fp contract(off)   /* multiply and add rounded separately, as the reference's two tensor operations */
        const float *s = xy + i * 10;
        float v[10];
#pragma unroll
        for (int k = 0; k < 10; ++k)
            v[k] = hf_nan_to_num(s[k]);
        float *d = box + i * 10;
        d[0] = v[0] * sx + x0; d[1] = v[1] * sy + y0; d[2] = v[3]; d[3] = v[4]; d[4] = v[2] * sz + z0;
        d[5] = v[5]; d[6] = v[6]; d[7] = v[7]; d[8] = v[8]; d[9] = v[9];
    }
}

extern "C" int rac_head_finish_fwd(float *cls, int64_t n_cls, const float *xy, float *box, int64_t rows, int code_size,
                                   const float *pc_range, void *stream)
{
    RAC_CHECK_ARG(n_cls >= 0 && rows >= 0 && code_size == 10, "rac_head_finish_fwd: n_cls=%lld rows=%lld code_size=%d (10)",
                  (long long)n_cls, (long long)rows, code_size);
    const long n = n_cls > rows ? n_cls : rows;
    if (n == 0)
        return 0;
    RAC_CHECK_ARG((cls || n_cls == 0) && (rows == 0 || (xy && box)) && pc_range && xy != box, "rac_head_finish_fwd: null pointer or xy aliases box");
    hipLaunchKernelGGL(head_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, cls, (long)n_cls, xy, box,
                       (long)rows, pc_range[0], pc_range[1], pc_range[2], pc_range[3] - pc_range[0], pc_range[4] - pc_range[1],
                       pc_range[5] - pc_range[2]);
    return rac_launch_status("rac_head_finish_fwd");
}

// ------------------------------------------------------------------------------------------------ layer boundary
// One launch at the boundary between two decoder layers: refine_bbox of the finished layer (as refine_kernel) and, for
// the boxes it produces, what the next layer computes first: the per-query box table (box_prep_kernel) and the head of the
// position encoder relu(LN(W x + b)) on (theta, d, z) (pe_head_kernel).  One wave per query: every lane evaluates the
// (cheap, identical) box arithmetic, lane 0 stores it, then the wave does the 256-wide LayerNorm.
__device__ __forceinline__ float lb_wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(256) void layer_boundary_kernel(const float *__restrict__ prop, const float *__restrict__ delta,
                                                             const float *__restrict__ td_safe, float *__restrict__ pred,
                                                             float *__restrict__ xy, float *__restrict__ table,
                                                             const float *__restrict__ W, const float *__restrict__ bias,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta,
                                                             float *__restrict__ h_out, int n, int Q, int T, float num_ray,
                                                             float eps, float p0, float p1, float p2, float sx, float sy, float sz)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (i >= n)
        return;
    const float *p = prop + (size_t)i * 10, *d = delta + (size_t)i * 10;
    float o[10];
    o[0] = p[0] + (ref_sigmoid(d[0]) * 2.f - 1.f) / num_ray;
    o[1] = ref_sigmoid(d[1] + ref_inverse_sigmoid(p[1]));
    o[2] = ref_sigmoid(d[2] + ref_inverse_sigmoid(p[2]));
#pragma unroll
    for (int k = 3; k < 10; ++k)
        o[k] = d[k];
    if (T > 1) {
        const float td = td_safe[(i / Q) * T + 1];
        o[8] = o[8] / td;
        o[9] = o[9] / td;
    }
    const float ang = o[0] * REF_TWO_PI, rad = o[1] * 65.0f;
    const float xn = fminf(fmaxf((51.2f + rad * cosf(ang)) / 102.4f, 0.f), 1.f);
    const float yn = fminf(fmaxf((51.2f + rad * sinf(ang)) / 102.4f, 0.f), 1.f);
    if (lane == 0) {
        float *pp = pred + (size_t)i * 10, *px = xy + (size_t)i * 10, *t = table + (size_t)i * 8;
#pragma unroll
        for (int k = 0; k < 10; ++k)
            pp[k] = o[k];
        px[0] = xn;
        px[1] = yn;
#pragma unroll
        for (int k = 2; k < 10; ++k)
            px[k] = o[k];
        const float yaw = atan2f(o[6], o[7]);
        t[0] = xn * sx + p0;
        t[1] = yn * sy + p1;
        t[2] = o[2] * sz + p2;
        t[3] = expf(o[3]);
        t[4] = expf(o[4]);
        t[5] = expf(o[5]);
        t[6] = cosf(yaw);
        t[7] = sinf(yaw);
    }
    // position-encoder head on (theta, d, z) of the refined box (as pe_head_kernel)
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = lane * 4 + j;
        v[j] = W[c * 3] * o[0] + W[c * 3 + 1] * o[1] + W[c * 3 + 2] * o[2] + bias[c];
    }
    const float mean = lb_wave_sum((v[0] + v[1]) + (v[2] + v[3])) / 256.f;
    const float d0 = v[0] - mean, d1 = v[1] - mean, d2 = v[2] - mean, d3 = v[3] - mean;
    const float rstd = 1.f / sqrtf(lb_wave_sum((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) / 256.f + eps);
    const rac_f4 g = rac_ld4(gamma + lane * 4), b = rac_ld4(beta + lane * 4);
    rac_f4 y = {rac_relu(d0 * rstd * g.x + b.x), rac_relu(d1 * rstd * g.y + b.y), rac_relu(d2 * rstd * g.z + b.z),
                rac_relu(d3 * rstd * g.w + b.w)};
    *reinterpret_cast<rac_f4 *>(h_out + (size_t)i * 256 + lane * 4) = y;
}

extern "C" int rac_layer_boundary_fwd(const float *proposal, const float *delta, const float *time_diff_safe, float *bbox_pred,
                                      float *bbox_xy, float *box_table, const float *pc_range, const float *pe_weight,
                                      const float *pe_bias, const float *pe_gamma, const float *pe_beta, float *pe_out, int B,
                                      int Q, int T, int dim, float num_ray, float eps, void *stream)
{
    RAC_CHECK_ARG(B >= 0 && Q >= 0 && T >= 1 && num_ray > 0.f && dim == 256, "rac_layer_boundary_fwd: bad sizes B=%d Q=%d T=%d dim=%d", B, Q, T, dim);
    if (B * Q == 0)
        return 0;
    RAC_CHECK_ARG(proposal && delta && time_diff_safe && bbox_pred && bbox_xy && box_table && pc_range && pe_weight && pe_bias &&
                      pe_gamma && pe_beta && pe_out,
                  "rac_layer_boundary_fwd: null pointer");
    const int n = B * Q;
    hipLaunchKernelGGL(layer_boundary_kernel, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, proposal, delta,
                       time_diff_safe, bbox_pred, bbox_xy, box_table, pe_weight, pe_bias, pe_gamma, pe_beta, pe_out, n, Q, T,
                       num_ray, eps, pc_range[0], pc_range[1], pc_range[2], pc_range[3] - pc_range[0], pc_range[4] - pc_range[1],
                       pc_range[5] - pc_range[2]);
    return rac_launch_status("rac_layer_boundary_fwd");
}
