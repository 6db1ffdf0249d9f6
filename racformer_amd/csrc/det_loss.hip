// det_loss.hip -- the head's classification and box losses of all decoder layers in ONE launch (gfx950): sigmoid focal loss
// plus code-weighted L1 against normalize_bbox of each row's ground-truth box, forward sums and unit gradients in the same
// pass.  Replaces, per layer, the target scatter of _get_target_single, FocalLoss and L1Loss with their autograd backwards
// (models/racformer_head.py:264-300, 326-427: one_hot, sigmoid, BCE, pow, masks, boolean row selection, abs, sums -- some
// thirty torch launches a layer, forward and backward).
//
// Rows: [L][R].  A row's target is entry tgt[l][r] of the concatenated ground-truth table (-1: background), or, with tgt
// NULL, entry r mod num_gt (the denoising rows that prepare_for_dn_loss gathers).  The label of a background row is
// num_classes (an all-zero one-hot); its box term is skipped; a positive row's box term is skipped when normalize_bbox of
// its box has a non-finite entry (the reference's isnotnan).
//
// One workgroup of 1024 threads per layer.  Each thread sums its elements in index order in float64, the workgroup adds the
// 1024 partial sums in a fixed tree in LDS: no float atomics, two runs give the same bits.  These are small, latency-bound
// kernels -- what they buy is the launch count.
#include "rac_common.h"

#define DL_THREADS 1024

struct DetLossArgs {
    const float *logits;   // [L][R][C]
    const float *boxes;    // [L][R][10]
    const int *tgt;        // [L][R] or NULL
    const float *gt;       // [num_gt][9]
    const int *labels;     // [num_gt]
    const float *cw;       // [10]
    float *sums;           // [L][2]: classification, box
    float *g_logits;       // [L][R][C]
    float *g_boxes;        // [L][R][10]
    int R, C, num_gt;
    float alpha, gamma;
};

__device__ __forceinline__ float dl_pow(float x, float gamma)
{
    return gamma == 2.f ? x * x : powf(x, gamma);
}

__global__ __launch_bounds__(DL_THREADS) void det_loss_kernel(const DetLossArgs a)
{
    __shared__ double red[2][DL_THREADS];
    const int l = blockIdx.x, tid = threadIdx.x;
    const int R = a.R, C = a.C;
    const float *logits = a.logits + (size_t)l * R * C;
    float *g_logits = a.g_logits + (size_t)l * R * C;
    const int *tgt = a.tgt ? a.tgt + (size_t)l * R : nullptr;
    double s_cls = 0.0, s_box = 0.0;

    // sigmoid focal loss, one element per thread and trip: loss = BCE_with_logits(x, t) * (alpha t + (1 - alpha)(1 - t)) * pt^gamma
    const long n_el = (long)R * C;
    for (long e = tid; e < n_el; e += DL_THREADS) {
        const int row = (int)(e / C), c = (int)(e - (long)row * C);
        int ti = tgt ? tgt[row] : (a.num_gt > 0 ? row % a.num_gt : -1);
        if (ti >= a.num_gt)
            ti = -1;
        const int label = ti >= 0 ? a.labels[ti] : C;
        const float x = logits[e];
        const float en = expf(-fabsf(x)), sp = log1pf(en), inv = 1.f / (1.f + en);
        const float p = x >= 0.f ? inv : en * inv, q1 = x >= 0.f ? en * inv : inv;       // sigmoid(x), 1 - sigmoid(x)
        float loss, grad;
        if (c == label) {
            const float bce = fmaxf(-x, 0.f) + sp, fw = a.alpha * dl_pow(q1, a.gamma);   // -log p
            loss = bce * fw;
            grad = fw * (-a.gamma * p * bce - q1);
        } else {
            const float bce = fmaxf(x, 0.f) + sp, fw = (1.f - a.alpha) * dl_pow(p, a.gamma);   // -log(1 - p)
            loss = bce * fw;
            grad = fw * (a.gamma * q1 * bce + p);
        }
        g_logits[e] = grad;
        s_cls += (double)loss;
    }

    // L1 against the code-weighted normalised box, one row per thread and trip
    float cw[10];
#pragma unroll
    for (int k = 0; k < 10; ++k)
        cw[k] = a.cw[k];
    for (int row = tid; row < R; row += DL_THREADS) {
        int ti = tgt ? tgt[row] : (a.num_gt > 0 ? row % a.num_gt : -1);
        if (ti >= a.num_gt)
            ti = -1;
        float *g = a.g_boxes + ((size_t)l * R + row) * 10;
        bool use = ti >= 0;
        float nb[10];
        if (use) {
            const float *t = a.gt + (size_t)ti * 9;
            nb[0] = t[0]; nb[1] = t[1]; nb[2] = logf(t[3]); nb[3] = logf(t[4]); nb[4] = t[2]; nb[5] = logf(t[5]);
            nb[6] = sinf(t[6]); nb[7] = cosf(t[6]); nb[8] = t[7]; nb[9] = t[8];
#pragma unroll
            for (int k = 0; k < 10; ++k)
                use = use && isfinite(nb[k]);
        }
        if (!use) {
#pragma unroll
            for (int k = 0; k < 10; ++k)
                g[k] = 0.f;
            continue;
        }
        const float *pb = a.boxes + ((size_t)l * R + row) * 10;
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            const float d = pb[k] - nb[k];
            s_box += (double)(fabsf(d) * cw[k]);
            g[k] = d > 0.f ? cw[k] : (d < 0.f ? -cw[k] : 0.f);
        }
    }

    red[0][tid] = s_cls;
    red[1][tid] = s_box;
    __syncthreads();
    for (int half = DL_THREADS / 2; half >= 1; half >>= 1) {
        if (tid < half) {
            red[0][tid] += red[0][tid + half];
            red[1][tid] += red[1][tid + half];
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.sums[l * 2 + 0] = (float)red[0][0];
        a.sums[l * 2 + 1] = (float)red[1][0];
    }
}

extern "C" int rac_det_loss_fwd(const float *logits, const float *boxes, const int32_t *target, const float *gt_boxes,
                                const int32_t *gt_labels, const float *code_weights, float *sums, float *grad_logits, float *grad_boxes,
                                int num_layers, int rows, int num_classes, int num_gt, float alpha, float gamma, void *stream)
{
    RAC_CHECK_ARG(num_layers >= 0 && rows >= 0 && num_classes >= 1 && num_gt >= 0, "rac_det_loss_fwd: L=%d rows=%d C=%d num_gt=%d", num_layers,
                  rows, num_classes, num_gt);
    if (num_layers == 0)
        return 0;
    RAC_CHECK_ARG(sums && code_weights, "rac_det_loss_fwd: null pointer");
    RAC_CHECK_ARG(rows == 0 || (logits && boxes && grad_logits && grad_boxes), "rac_det_loss_fwd: null pointer");
    RAC_CHECK_ARG(num_gt == 0 || (gt_boxes && gt_labels), "rac_det_loss_fwd: null pointer");
    DetLossArgs a;
    a.logits = logits; a.boxes = boxes; a.tgt = target; a.gt = gt_boxes; a.labels = gt_labels; a.cw = code_weights;
    a.sums = sums; a.g_logits = grad_logits; a.g_boxes = grad_boxes;
    a.R = rows; a.C = num_classes; a.num_gt = num_gt; a.alpha = alpha; a.gamma = gamma;
    hipLaunchKernelGGL(det_loss_kernel, dim3(num_layers), dim3(DL_THREADS), 0, (hipStream_t)stream, a);
    return rac_launch_status("rac_det_loss_fwd");
}
