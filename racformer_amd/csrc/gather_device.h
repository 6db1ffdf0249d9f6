// gather_device.h -- what the msmv and MSDA gathers (msmv_fwd.hip, msmv_bwd.hip, msmv_v2.hip, msda_fwd.hip, msda_bwd.hip)
// decide alike: the bilinear footprint of a sample, the camera of an msmv point, the slot order of [B,Q,G,T*P,C], the
// 16-lane group sum, the f32 / bf16 loads, and the msmv kernel arguments with their host checks.  Each kernel keeps its
// own tap offsets, accumulation order and launch shape.
#pragma once
#include "rac_common.h"

#define RAC_TAP_OUTSIDE 0x80000000u   /* tap byte offset past the end of a buffer descriptor's range: the load returns zeros */
typedef unsigned int rac_u2 __attribute__((ext_vector_type(2)));
typedef unsigned int rac_u4 __attribute__((ext_vector_type(4)));

// Bilinear footprint of a sample at pixel coordinates (h_im, w_im) of an H x W map: msmv passes v*(H-1), u*(W-1)
// (align_corners=True), MSDA y*H - 0.5, x*W - 0.5 (align_corners=False).  As in the reference kernels the sample counts
// only if h_im > -1 && w_im > -1 && h_im < H && w_im < W (`in`), and each tap only inside the map (`ok`).  Outside the guard
// the footprint is pinned to (0, 0): a NaN / inf coordinate then gives finite tap weights (NaN times a zero tap would be
// NaN), and a huge one never reaches the float -> int conversion.
// Differences rounded one by one, as the reference's statements read and as the oracle computes them: a contracted
// fma(v, H-1, -floor) would move a weight by an ulp of the pixel coordinate -- 1e-5 of a pixel at W = 176.
struct RacFootprint {
    int h_low, w_low;
    float lh, lw, hh, hw;
    bool in;
    bool ok[4];   // top-left, top-right, bottom-left, bottom-right inside the map (all false unless `in`)
};
__device__ __forceinline__ RacFootprint rac_footprint(float h_im, float w_im, int H, int W)
{
#pragma clang fp contract(off)
    RacFootprint f;
    f.in = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
    const float h = f.in ? h_im : 0.f, w = f.in ? w_im : 0.f;   // (the pin as two selects on the inputs: no branch)
    const float hf = floorf(h), wf = floorf(w);
    f.h_low = (int)hf;
    f.w_low = (int)wf;
    f.lh = h - hf;
    f.lw = w - wf;
    f.hh = 1.f - f.lh;
    f.hw = 1.f - f.lw;
    const bool top = f.in && f.h_low >= 0, bot = f.in && f.h_low + 1 <= H - 1;
    const bool left = f.w_low >= 0, right = f.w_low + 1 <= W - 1;
    f.ok[0] = top && left;
    f.ok[1] = top && right;
    f.ok[2] = bot && left;
    f.ok[3] = bot && right;
    return f;
}

// camera of an msmv point: round(z * (N-1)) (half away from zero, as C round) clamped to [0, N-1]
__device__ __forceinline__ int rac_msmv_view(float z, int N)
{
    const int view = (int)roundf(z * (float)(N - 1));
    return min(max(view, 0), N - 1);
}

__device__ __forceinline__ float rac_group_sum16(float v)
{
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1)
        v += __shfl_xor(v, off, 16);
    return v;
}

template <typename FT>
__device__ __forceinline__ float rac_ld1(const FT *p)
{
    if constexpr (sizeof(FT) == 4)
        return *p;
    else
        return rac_bf16_to_f32(*p);
}

// Four channels of one tap through a buffer descriptor: its range check stands in for the four branches of the bilinear
// footprint (a tap outside the map carries the offset RAC_TAP_OUTSIDE and reads as zero).  AUX: cache policy of the load
// (0 default, 2 = nt).
template <typename FT, int AUX = 0>
__device__ __forceinline__ rac_f4 rac_tap(__amdgpu_buffer_rsrc_t rsrc, unsigned off)
{
    if constexpr (sizeof(FT) == 4) {
        return __builtin_bit_cast(rac_f4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, AUX));
    } else {
        const rac_u2 r = __builtin_amdgcn_raw_buffer_load_b64(rsrc, off, 0, AUX);    // 4 x bf16
        return (rac_f4){__uint_as_float(r.x << 16), __uint_as_float(r.x & 0xffff0000u), __uint_as_float(r.y << 16),
                        __uint_as_float(r.y & 0xffff0000u)};
    }
}

// ---- msmv (rac_msmv_fwd / _bwd, rac_msmv_v2_fwd / _bwd): one argument block for every kernel
struct MsmvArgs {
    const void *feat[RAC_MAX_LEVELS];
    float *gfeat[RAC_MAX_LEVELS];          // backwards
    int H[RAC_MAX_LEVELS];
    int W[RAC_MAX_LEVELS];
    unsigned feat_bytes[RAC_MAX_LEVELS];   // one slot's N maps of each level (the buffer descriptors' ranges; rac_msmv_fwd C = 64)
    const float *loc;       // [S,Q,P,3]
    const float *w;         // [S,Q,P,L]
    const float *grad_out;  // layout by T (backwards)
    float *out;             // layout by T (forwards)
    float *gloc;            // [S,Q,P,3]   (backwards)
    float *gw;              // [S,Q,P,L]   (rac_msmv_bwd)
    int L, S, N, Q, P, C;
    int T, G;               // T > 0: RAC_OUT_BQGTPC [B,Q,G,T*P,C], slot s = (b*T + t)*G + g; T = 0: RAC_OUT_SQCP [S,Q,C,P]
    int cf;                 // 1: features [S,C,N,H,W] (rac_msmv_v2_*)
    int blocks_per_slot;    // rac_msmv_fwd C = 64
};

// output / gradient element of channel c of point p of row (s, q), and the distance between consecutive channels
struct RacOutIdx {
    size_t base, cstride;
};
__device__ __forceinline__ RacOutIdx msmv_out_index(const MsmvArgs &a, bool bqgtpc, int s, int q, int p, int c = 0)
{
    if (bqgtpc) {
        const int g = s % a.G, t = (s / a.G) % a.T, b = s / (a.G * a.T);
        return RacOutIdx{(((((size_t)b * a.Q + q) * a.G + g) * a.T + t) * a.P + p) * a.C + c, 1};
    }
    return RacOutIdx{((((size_t)s * a.Q + q) * a.C + c) * a.P + p), (size_t)a.P};
}

enum MsmvEntry { MSMV_FWD, MSMV_BWD, MSMV_V2_FWD, MSMV_V2_BWD };

// Fills `a` from the arguments of an msmv entry point, with that entry point's checks in its order, all before the first
// HIP call.  Returns RAC_E_ARG (rac_last_error set) or 0; nothing to launch (S, Q or P = 0) returns 0 with a.S = 0.
// `layout`: the output layout of a forward, the gradient's of a backward.  `io`: the entry point's own output pointers
// are set (out; grad_out, grad_loc and for rac_msmv_bwd grad_w); the entry point stores them in `a` afterwards.  The
// dtype and feature-layout checks sit here only because their place in the order differs between the entry points;
// feat_bytes and the choice of kernel stay with the entry point.
static int msmv_fill_args(MsmvArgs &a, MsmvEntry e, const char *what, int layout, int T, int G, const void *const *feats,
                          void *const *grad_feats, const int32_t *hw, int L, const float *loc, const float *w, bool io,
                          int S, int N, int Q, int P, int C, int dtype, int feat_layout)
{
    const bool bwd = e == MSMV_BWD || e == MSMV_V2_BWD, v2 = e == MSMV_V2_FWD || e == MSMV_V2_BWD;
    a.S = 0;
    RAC_CHECK_ARG(L >= 1 && L <= RAC_MAX_LEVELS, "%s: L=%d out of [1,%d]", what, L, RAC_MAX_LEVELS);
    RAC_CHECK_ARG(S >= 0 && Q >= 0 && N >= 1 && C >= 1, "%s: bad sizes S=%d N=%d Q=%d C=%d", what, S, N, Q, C);
    RAC_CHECK_ARG(P >= 0 && P <= RAC_MAX_POINTS, "%s: num_point exceed limits (P=%d > %d)", what, P, RAC_MAX_POINTS);
    const bool empty = S == 0 || Q == 0 || P == 0;
    if (e == MSMV_FWD) {   // (rac_msmv_fwd: the empty return and the pointers come before its dtype and layout)
        if (empty)
            return 0;
        RAC_CHECK_ARG(feats && hw && loc && w && io, "%s: null pointer", what);
    }
    if (!bwd)
        RAC_CHECK_ARG(dtype == RAC_F32 || dtype == RAC_BF16, "%s: dtype %d", what, dtype);
    if (v2)
        RAC_CHECK_ARG(feat_layout == RAC_FEAT_CL || feat_layout == RAC_FEAT_CF, "%s: feature layout %d", what, feat_layout);
    if (e == MSMV_V2_FWD)
        RAC_CHECK_ARG(feat_layout == RAC_FEAT_CL || dtype == RAC_F32, "%s: channel-first features are float32 only", what);
    RAC_CHECK_ARG(layout == RAC_OUT_SQCP || layout == RAC_OUT_BQGTPC, bwd ? "%s: gradient layout %d" : "%s: layout %d", what,
                  layout);
    if (bwd)
        RAC_CHECK_ARG(T >= 1 && G >= 1, "%s: T=%d G=%d must be >= 1", what, T, G);
    if (layout == RAC_OUT_BQGTPC)
        RAC_CHECK_ARG(T >= 1 && G >= 1 && S % (T * G) == 0, "%s: S=%d not a multiple of T*G=%d*%d", what, S, T, G);
    if (empty)
        return 0;   // nothing to launch (torch hands out null data pointers for empty tensors)
    RAC_CHECK_ARG(io && hw && feats && (!bwd || grad_feats) && (v2 || (loc && w)), "%s: null pointer", what);
    for (int l = 0; l < RAC_MAX_LEVELS; ++l) {
        a.feat[l] = nullptr;
        a.gfeat[l] = nullptr;
        a.H[l] = a.W[l] = 1;
        a.feat_bytes[l] = 0;
    }
    for (int l = 0; l < L; ++l) {
        const bool ptr_ok = feats[l] != nullptr && (!bwd || grad_feats[l] != nullptr);
        const bool map_ok = hw[2 * l] >= 1 && hw[2 * l + 1] >= 1;
        if (e == MSMV_FWD) {
            RAC_CHECK_ARG(ptr_ok, "%s: feats[%d] is null", what, l);
            RAC_CHECK_ARG(map_ok, "%s: level %d has empty map", what, l);
        } else if (e == MSMV_BWD) {
            RAC_CHECK_ARG(ptr_ok && map_ok, "%s: level %d", what, l);
        } else {
            RAC_CHECK_ARG(ptr_ok, "%s: level %d pointer is null", what, l);
            RAC_CHECK_ARG(map_ok, "%s: level %d has an empty map", what, l);
        }
        a.feat[l] = feats[l];
        a.gfeat[l] = bwd ? (float *)grad_feats[l] : nullptr;
        a.H[l] = hw[2 * l];
        a.W[l] = hw[2 * l + 1];
    }
    RAC_CHECK_ARG(loc && w, "%s: null pointer", what);
    a.loc = loc; a.w = w;
    a.grad_out = nullptr; a.out = nullptr; a.gloc = nullptr; a.gw = nullptr;
    a.L = L; a.S = S; a.N = N; a.Q = Q; a.P = P; a.C = C;
    a.T = layout == RAC_OUT_BQGTPC ? T : 0;
    a.G = layout == RAC_OUT_BQGTPC ? G : 1;
    a.cf = feat_layout == RAC_FEAT_CF;
    a.blocks_per_slot = 0;
    return 0;
}
