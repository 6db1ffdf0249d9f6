// bev_device.h -- what the BEV sampling forward (bev_fused.hip) and its backward (bev_fused_bwd.hip) compute alike: the
// T-invariant base point of a keypoint, the ray-depth offset, the two wave softmaxes, the per-frame warp with its polar
// jitter, and the whole chain from the query box as it is formed for B > 1.  The backward recomputes the keypoints with these functions instead of reading saved ones, so its locations and
// weights are the forward's own.
#pragma once
#include "rac_common.h"

#define BEV_MAX_DEPTH 16
#define BEV_TWO_PI 6.283185307179586f

// polar jitter of a keypoint (racformer_transformer.py:512-522 through models/bbox/utils.py:84-106): (ex, ey) metres from the
// map centre -> (dist, theta), dist += doff, back to the normalised map.  (Scaling the unit vector (ex, ey) / r directly
// would skip atan2f / fmodf / cosf / sinf; measured: under 1 us of 81 per launch -- not worth leaving the reference's chain.)
__device__ __forceinline__ void bev_polar_jitter(float ex, float ey, float doff, float *loc2)
{
    const float dist = sqrtf(ex * ex + ey * ey) / 65.0f + doff;
    const float th = fmodf(atan2f(ey, ex) + BEV_TWO_PI, BEV_TWO_PI) / BEV_TWO_PI;
    const float ang = th * BEV_TWO_PI, rad = dist * 65.0f;
    loc2[0] = fminf(fmaxf((51.2f + rad * cosf(ang)) / 102.4f, 0.f), 1.f);
    loc2[1] = fminf(fmaxf((51.2f + rad * sinf(ang)) / 102.4f, 0.f), 1.f);
}

// T-invariant base point of keypoint (h, p): box centre + R(yaw) (exp(w, l) * offset).  bt: the query's row of the box table
// (rac_box_prep_fwd; entries 0, 1, 3, 4, 6, 7 are read)
// The two fused multiply-adds are written out, with contraction off: left to the compiler, dx * sin + dy * cos became
// fma(dy, cos, dx * sin) in the forward kernel and fma(dx, sin, dy * cos) in the backward -- an ulp apart for one base point in
// a few hundred, which the polar jitter turns into up to 7 ulps of the location.  This is the forward's form.
__device__ __forceinline__ void bev_base_point(const float *bt, float o0, float o1, float *base2)
{
#pragma clang fp contract(off)
    const float dx = bt[3] * o0, dy = bt[4] * o1;
    base2[0] = bt[0] + __builtin_fmaf(dx, bt[6], -(dy * bt[7]));
    base2[1] = bt[1] + __builtin_fmaf(dy, bt[6], dx * bt[7]);
}

__device__ __forceinline__ float bev_sigmoid(float x)
{
    return 1.f / (1.f + expf(-x));
}
// distance offset of depth slot d: its base + the learned shift inside the slot (sg = sigmoid of the ray logit)
__device__ __forceinline__ float bev_depth_offset(float sg, float depth_base, float d_region, int D)
{
    return depth_base + (sg * 2.f - 1.f) * d_region / (float)D / 2.f;
}

// per-(t,p) half of the keypoint chain for B==1: warp the T-invariant base point, polar jitter.
__device__ __forceinline__ void bev_warp(const float *pc, float px, float py, float vx, float vy, float td,
                                         float doff, float *loc2)
{
    const float sx = pc[3] - pc[0], sy = pc[4] - pc[1];
    px -= vx * td;
    py -= vy * td;
    const float nx = (px - pc[0]) / sx, ny = (py - pc[1]) / sy;
    const float ex = nx * 102.4f - 51.2f, ey = ny * 102.4f - 51.2f;
    bev_polar_jitter(ex, ey, doff, loc2);
}

// The whole keypoint chain of one (query, head, point, frame) from the query box itself, as the forward forms it for B > 1
// (no box table, no T-invariant half: the frame / batch pairing reads another sample's query per frame).  qb: the query's
// [10] row, o: the point's two offsets, td: the frame's time difference.  The rotation's two multiply-adds are written out with
// contraction off, for the reason given at bev_base_point: this is the form the forward kernel was compiled to.
__device__ __forceinline__ void bev_keypoint_from_query(const float *pc, const float *qb, const float *o, float ray_logit, float td,
                                                        float depth_base, float d_region, int D, float *loc2)
{
    const float sx = pc[3] - pc[0], sy = pc[4] - pc[1];
    const float ang0 = qb[0] * BEV_TWO_PI, rad0 = qb[1] * 65.0f;
    const float xn0 = fminf(fmaxf((51.2f + rad0 * cosf(ang0)) / 102.4f, 0.f), 1.f);
    const float yn0 = fminf(fmaxf((51.2f + rad0 * sinf(ang0)) / 102.4f, 0.f), 1.f);
    const float cx = xn0 * sx + pc[0], cy = yn0 * sy + pc[1];
    const float yaw = atan2f(qb[6], qb[7]);
    const float cs = cosf(yaw), sn = sinf(yaw);
    const float dx = expf(qb[3]) * o[0], dy = expf(qb[4]) * o[1];
    float rx, ry;
    {
#pragma clang fp contract(off)
        rx = __builtin_fmaf(dx, cs, -(dy * sn));
        ry = __builtin_fmaf(dx, sn, dy * cs);
    }
    float px = cx + rx;
    float py = cy + ry;
    px -= qb[8] * td;
    py -= qb[9] * td;
    const float nx = (px - pc[0]) / sx, ny = (py - pc[1]) / sy;
    const float ex = nx * 102.4f - 51.2f, ey = ny * 102.4f - 51.2f;
    const float sg = 1.f / (1.f + expf(-ray_logit));
    bev_polar_jitter(ex, ey, depth_base + (sg * 2.f - 1.f) * d_region / (float)D / 2.f, loc2);
}

__device__ __forceinline__ float bev_wave_max(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        v = fmaxf(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ float bev_wave_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1)
        v += __shfl_xor(v, m, 64);
    return v;
}

// softmax across the lanes of a wave: lanes with `live` hold a logit, the others -INFINITY; returns the lane's weight
__device__ __forceinline__ float bev_wave_softmax(float logit, bool live)
{
    const float m = bev_wave_max(logit);
    const float e = live ? expf(logit - m) : 0.f;
    return e / bev_wave_sum(e);
}
