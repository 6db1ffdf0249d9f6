// msmv_v2.hip -- hard-level multi-scale multi-view sampling (msmv_sampling_v2), forward and backward, for gfx950 (MI355X).
//
// Replaces the reference's torch-only msmv_sampling_pytorch_v2 (models/csrc/wrapper.py:41-76) behind rac_msmv_v2_fwd /
// rac_msmv_v2_bwd.  Per point (s, q, p):
//   l*   = argmax_l w[s,q,p,l] with torch.argmax's rules (first maximal index wins a tie, a NaN counts as maximal so the
//          first NaN wins, an all -inf row gives 0)
//   view = round(loc_z * (N-1)) clamped to [0, N-1]                                      (as rac_msmv_fwd)
//   out  = bilinear0(feats[l*][s, view], u*(W-1), v*(H-1)), align_corners=True, zero padding, NOT scaled by w
// The reference samples all L levels with grid_sample, stacks them and keeps the argmax level; here the level is chosen
// first and only its 4 taps are read: 1/L of rac_msmv_fwd's gathers.  The argmax runs in the kernel (no one-hot, no host
// sync, no allocation: capturable in a graph).
// Backward (fp32): grad_feat[l*][tap] += w_tap * grad_out (float atomics into a caller-zeroed buffer);
//   grad_loc (u, v) = (W_l*-1 | H_l*-1) * sum_c grad_out[c] * d bilinear[c] / d(w|h), one writer per point (deterministic);
//   grad_loc view = 0 (as rac_msmv_bwd); the weights get no gradient (argmax cuts the graph in the reference too).
//   grad_out in either output layout (rac_msmv_v2_bwd_ex): [S,Q,C,P], or [B,Q,G,T*P,C] as the forward writes it for
//   sampling_4d, where a point's 64 channels are one contiguous row (the C = 64 kernel's lanes read floats c + 16 j of it).
//
// Feature layouts: RAC_FEAT_CL [S,N,H,W,C] (the package's pyramid, what the decoder hands the op) and RAC_FEAT_CF
// [S,C,N,H,W] (what the reference's torch path takes; fp32).
//  * C = 64, channel-last: a 16-lane group owns one point, each lane 4 channels; forward taps are one 16-byte (f32) or
//    8-byte (bf16) load per lane, 256 contiguous bytes per point.  The backward stripes a lane's channels c, c+16, c+32,
//    c+48 (as msmv_bwd.hip) so that each atomic wave-instruction adds four whole 64-byte segments.
//  * any other C, and channel-first: one thread per (point, channel) forward, one thread per point backward, through a
//    stride table that covers both layouts.
#include "gather_device.h"

// torch.argmax over a weight row: ties -> first index, NaN is maximal (first NaN wins), all -inf -> 0
__device__ __forceinline__ int v2_argmax(const float *wp, int L)
{
    int best = 0;
    float bw = wp[0];
#pragma unroll
    for (int l = 1; l < RAC_MAX_LEVELS; ++l) {
        if (l < L) {
            const float x = wp[l];
            if (bw == bw && (x > bw || x != x)) {
                best = l;
                bw = x;
            }
        }
    }
    return best;
}

// the chosen level's map pointer and size out of the kernel arguments (a compare-select chain over the levels: the
// argument words stay scalar, no dynamic indexing of the kernarg block)
struct V2Level {
    const void *feat;
    float *gfeat;
    int H, W;
};
__device__ __forceinline__ V2Level v2_level(const MsmvArgs &a, int lsel)
{
    V2Level r{a.feat[0], a.gfeat[0], a.H[0], a.W[0]};
#pragma unroll
    for (int l = 1; l < RAC_MAX_LEVELS; ++l) {
        const bool take = l == lsel;
        r.feat = take ? a.feat[l] : r.feat;
        r.gfeat = take ? a.gfeat[l] : r.gfeat;
        r.H = take ? a.H[l] : r.H;
        r.W = take ? a.W[l] : r.W;
        // (kept as selects: left alone, hipcc turns the chain back into a dynamic index into a stack copy of the arrays)
        asm volatile("" : "+v"(r.H), "+v"(r.W));
    }
    return r;
}

// footprint of a point on the chosen level (align_corners=True)
__device__ __forceinline__ RacFootprint v2_footprint(float lu, float lv, int H, int W)
{
    return rac_footprint(lv * (float)(H - 1), lu * (float)(W - 1), H, W);
}

// ---- forward, C = 64, channel-last: one 16-lane group per point, 4 adjacent channels per lane
template <typename FT>
__global__ __launch_bounds__(256) void msmv_v2_fwd_c64_kernel(const MsmvArgs a)
{
    const int c4 = threadIdx.x & 15;
    const long pt = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;   // (s*Q + q)*P + p
    const long npts = (long)a.S * a.Q * a.P;
    if (pt >= npts)
        return;
    const int p = (int)(pt % a.P);
    const long row = pt / a.P;
    const int s = (int)(row / a.Q);
    const float *lp = a.loc + pt * 3;
    const float lu = lp[0], lv = lp[1];
    const int view = rac_msmv_view(lp[2], a.N);
    const V2Level lv_ = v2_level(a, v2_argmax(a.w + pt * a.L, a.L));
    const RacFootprint t = v2_footprint(lu, lv, lv_.H, lv_.W);
    const FT *base = (const FT *)lv_.feat + ((size_t)s * a.N + view) * lv_.H * lv_.W * 64 + c4 * 4;
    const size_t pix[4] = {(size_t)t.h_low * lv_.W + t.w_low, (size_t)t.h_low * lv_.W + t.w_low + 1,
                           (size_t)(t.h_low + 1) * lv_.W + t.w_low, (size_t)(t.h_low + 1) * lv_.W + t.w_low + 1};
    rac_f4 v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        v[k] = t.ok[k] ? rac_ld4(base + pix[k] * 64) : (rac_f4){0.f, 0.f, 0.f, 0.f};
    float tw[4];
    {
#pragma clang fp contract(off)
        tw[0] = t.hh * t.hw;
        tw[1] = t.hh * t.lw;
        tw[2] = t.lh * t.hw;
        tw[3] = t.lh * t.lw;
    }
    rac_acc4 acc = rac_acc4_zero();
#pragma unroll
    for (int k = 0; k < 4; ++k)
        rac_tap_fma(acc, v[k].x, v[k].y, v[k].z, v[k].w, tw[k]);
    rac_f4 r;
    rac_acc4_get(acc, r.x, r.y, r.z, r.w);
    float *o = a.out + msmv_out_index(a, a.T > 0, s, (int)(row % a.Q), p, c4 * 4).base;
    if (a.T > 0) {
        *reinterpret_cast<rac_f4 *>(o) = r;
    } else {
        o[0] = r.x;
        o[(size_t)a.P] = r.y;
        o[(size_t)2 * a.P] = r.z;
        o[(size_t)3 * a.P] = r.w;
    }
}

// element strides of a map (s, view) of one level, in either layout: element (h, w, c) at map + (h*W + w)*pix + c*ch
struct V2Strides {
    size_t map, pix, ch;
};
__device__ __forceinline__ V2Strides v2_strides(const MsmvArgs &a, int s, int view, int H, int W)
{
    const size_t hw = (size_t)H * W;
    if (a.cf)   // [S,C,N,H,W]
        return V2Strides{((size_t)s * a.C * a.N + view) * hw, 1, (size_t)a.N * hw};
    return V2Strides{((size_t)s * a.N + view) * hw * a.C, (size_t)a.C, 1};   // [S,N,H,W,C]
}

// ---- forward, any C, either feature layout: one thread per (point, channel), channel fastest
template <typename FT>
__global__ __launch_bounds__(256) void msmv_v2_fwd_generic_kernel(const MsmvArgs a)
{
    const long total = (long)a.S * a.Q * a.P * a.C;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % a.C);
        const long pt = idx / a.C;
        const int p = (int)(pt % a.P);
        const long row = pt / a.P;
        const int s = (int)(row / a.Q), q = (int)(row % a.Q);
        const float *lp = a.loc + pt * 3;
        const int view = rac_msmv_view(lp[2], a.N);
        const V2Level lv_ = v2_level(a, v2_argmax(a.w + pt * a.L, a.L));
        const RacFootprint t = v2_footprint(lp[0], lp[1], lv_.H, lv_.W);
        const V2Strides st = v2_strides(a, s, view, lv_.H, lv_.W);
        const FT *base = (const FT *)lv_.feat + st.map + (size_t)c * st.ch;
        const size_t W = (size_t)lv_.W;
        const size_t pix[4] = {(size_t)t.h_low * W + t.w_low, (size_t)t.h_low * W + t.w_low + 1,
                               (size_t)(t.h_low + 1) * W + t.w_low, (size_t)(t.h_low + 1) * W + t.w_low + 1};
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
            v[k] = t.ok[k] ? rac_ld1(base + pix[k] * st.pix) : 0.f;
        float acc;
        {
#pragma clang fp contract(off)
            acc = t.hh * t.hw * v[0] + t.hh * t.lw * v[1] + t.lh * t.hw * v[2] + t.lh * t.lw * v[3];
        }
        a.out[msmv_out_index(a, a.T > 0, s, q, p, c).base] = acc;
    }
}

// ---- backward, C = 64, channel-last, fp32: one 16-lane group per point; lane c of the group owns channels c + 16 j
__global__ __launch_bounds__(256) void msmv_v2_bwd_c64_kernel(const MsmvArgs a)
{
    const int lane16 = threadIdx.x & 15;
    const long pt = ((long)blockIdx.x * 256 + threadIdx.x) >> 4;
    const long npts = (long)a.S * a.Q * a.P;
    const bool act = pt < npts;      // (no early return: the group sums below need all 16 lanes)
    const long ptc = act ? pt : 0;
    const int p = (int)(ptc % a.P);
    const long row = ptc / a.P;
    const int s = (int)(row / a.Q), q = (int)(row % a.Q);
    const float *lp = a.loc + ptc * 3;
    const int view = rac_msmv_view(lp[2], a.N);
    const V2Level lv_ = v2_level(a, v2_argmax(a.w + ptc * a.L, a.L));
    const int H = lv_.H, W = lv_.W;
    const RacFootprint t = v2_footprint(lp[0], lp[1], H, W);
    float g[4];
    {   // channel c of the point at go + c * cs: BQGTPC one contiguous 64-float row, SQCP P floats apart
        const RacOutIdx gi = msmv_out_index(a, a.T > 0, s, q, p, lane16);
        const float *go = a.grad_out + gi.base;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            g[j] = act ? go[(size_t)(16 * j) * gi.cstride] : 0.f;
    }
    const size_t map = ((size_t)s * a.N + view) * H * W * 64 + lane16;
    const float *base = (const float *)lv_.feat + map;
    float *gbase = lv_.gfeat + map;
    const size_t o[4] = {((size_t)t.h_low * W + t.w_low) * 64, ((size_t)t.h_low * W + t.w_low + 1) * 64,
                         ((size_t)(t.h_low + 1) * W + t.w_low) * 64, ((size_t)(t.h_low + 1) * W + t.w_low + 1) * 64};
    const float tw[4] = {t.hh * t.hw, t.hh * t.lw, t.lh * t.hw, t.lh * t.lw};
    const float dh[4] = {-t.hw, -t.lw, t.hw, t.lw}, dw[4] = {-t.hh, t.hh, -t.lh, t.lh};
    float sh = 0.f, sw_ = 0.f;   // this lane's share of sum_c grad_out[c] * d bilinear[c] / d(h | w)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool ok = act && t.ok[k];
        float v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = ok ? base[o[k] + 16 * j] : 0.f;
        if (ok) {   // per instruction the group adds 16 consecutive floats (64 bytes) of the tap's pixel row
#pragma unroll
            for (int j = 0; j < 4; ++j)
                atomicAdd(gbase + o[k] + 16 * j, tw[k] * g[j]);
        }
        const float dot = (v[0] * g[0] + v[1] * g[1]) + (v[2] * g[2] + v[3] * g[3]);
        sh += dh[k] * dot;
        sw_ += dw[k] * dot;
    }
    sh = rac_group_sum16(sh);
    sw_ = rac_group_sum16(sw_);
    if (act && lane16 == 0) {
        a.gloc[ptc * 3] = (float)(W - 1) * sw_;
        a.gloc[ptc * 3 + 1] = (float)(H - 1) * sh;
        a.gloc[ptc * 3 + 2] = 0.f;
    }
}

// ---- backward, any C, either feature layout, fp32: one thread per point, serial over the channels
__global__ __launch_bounds__(256) void msmv_v2_bwd_generic_kernel(const MsmvArgs a)
{
    const long npts = (long)a.S * a.Q * a.P;
    for (long pt = (long)blockIdx.x * blockDim.x + threadIdx.x; pt < npts; pt += (long)gridDim.x * blockDim.x) {
        const int p = (int)(pt % a.P);
        const long row = pt / a.P;
        const int s = (int)(row / a.Q), q = (int)(row % a.Q);
        const float *lp = a.loc + pt * 3;
        const int view = rac_msmv_view(lp[2], a.N);
        const V2Level lv_ = v2_level(a, v2_argmax(a.w + pt * a.L, a.L));
        const int H = lv_.H, W = lv_.W;
        const RacFootprint t = v2_footprint(lp[0], lp[1], H, W);
        const V2Strides st = v2_strides(a, s, view, H, W);
        const float *base = (const float *)lv_.feat + st.map;
        float *gbase = lv_.gfeat + st.map;
        const size_t o[4] = {((size_t)t.h_low * W + t.w_low) * st.pix, ((size_t)t.h_low * W + t.w_low + 1) * st.pix,
                             ((size_t)(t.h_low + 1) * W + t.w_low) * st.pix, ((size_t)(t.h_low + 1) * W + t.w_low + 1) * st.pix};
        const float tw[4] = {t.hh * t.hw, t.hh * t.lw, t.lh * t.hw, t.lh * t.lw};
        float sh = 0.f, sw_ = 0.f;
        if (t.in) {
            const RacOutIdx gi = msmv_out_index(a, a.T > 0, s, q, p);
            const float *go = a.grad_out + gi.base;
            const size_t gs = gi.cstride;
            for (int c = 0; c < a.C; ++c) {
                const float g = go[(size_t)c * gs];
                const size_t cc = (size_t)c * st.ch;
                float v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    v[k] = t.ok[k] ? base[o[k] + cc] : 0.f;
                    if (t.ok[k])
                        atomicAdd(gbase + o[k] + cc, tw[k] * g);
                }
                sh += (-t.hw * v[0] - t.lw * v[1] + t.hw * v[2] + t.lw * v[3]) * g;
                sw_ += (-t.hh * v[0] + t.hh * v[1] - t.lh * v[2] + t.lh * v[3]) * g;
            }
        }
        a.gloc[pt * 3] = (float)(W - 1) * sw_;
        a.gloc[pt * 3 + 1] = (float)(H - 1) * sh;
        a.gloc[pt * 3 + 2] = 0.f;
    }
}

extern "C" int rac_msmv_v2_fwd(const void *const *feats, const int32_t *hw, int L, const float *loc, const float *w,
                               float *out, int S, int N, int Q, int P, int C, int dtype, int feat_layout, int out_layout,
                               int T, int G, void *stream)
{
    MsmvArgs a;
    const int rc = msmv_fill_args(a, MSMV_V2_FWD, "rac_msmv_v2_fwd", out_layout, T, G, feats, nullptr, hw, L, loc, w,
                                  out != nullptr, S, N, Q, P, C, dtype, feat_layout);
    if (rc || a.S == 0)
        return rc;
    a.out = out;
    hipStream_t st = (hipStream_t)stream;
    const long npts = (long)S * Q * P;
    if (C == 64 && feat_layout == RAC_FEAT_CL) {
        const unsigned nb = (unsigned)((npts * 16 + 255) / 256);
        if (dtype == RAC_F32)
            hipLaunchKernelGGL(msmv_v2_fwd_c64_kernel<float>, dim3(nb), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL(msmv_v2_fwd_c64_kernel<unsigned short>, dim3(nb), dim3(256), 0, st, a);
    } else {
        const long total = npts * C;
        const int nb = (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
        if (dtype == RAC_F32)
            hipLaunchKernelGGL(msmv_v2_fwd_generic_kernel<float>, dim3(nb), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL(msmv_v2_fwd_generic_kernel<unsigned short>, dim3(nb), dim3(256), 0, st, a);
    }
    return rac_launch_status("rac_msmv_v2_fwd");
}

static int msmv_v2_bwd_impl(const char *what, const float *grad_out, int grad_layout, int T, int G, const void *const *feats,
                            const int32_t *hw, int L, const float *loc, const float *w, void *const *grad_feats, float *grad_loc,
                            int S, int N, int Q, int P, int C, int feat_layout, void *stream)
{
    MsmvArgs a;
    const int rc = msmv_fill_args(a, MSMV_V2_BWD, what, grad_layout, T, G, feats, grad_feats, hw, L, loc, w,
                                  grad_out && grad_loc, S, N, Q, P, C, RAC_F32, feat_layout);
    if (rc || a.S == 0)
        return rc;
    a.grad_out = grad_out;
    a.gloc = grad_loc;
    hipStream_t st = (hipStream_t)stream;
    const long npts = (long)S * Q * P;
    if (C == 64 && feat_layout == RAC_FEAT_CL) {
        const unsigned nb = (unsigned)((npts * 16 + 255) / 256);
        hipLaunchKernelGGL(msmv_v2_bwd_c64_kernel, dim3(nb), dim3(256), 0, st, a);
    } else {
        const unsigned nb = (unsigned)((npts + 255) / 256 > 4096 ? 4096 : (npts + 255) / 256);
        hipLaunchKernelGGL(msmv_v2_bwd_generic_kernel, dim3(nb), dim3(256), 0, st, a);
    }
    return rac_launch_status(what);
}

extern "C" int rac_msmv_v2_bwd_ex(const float *grad_out, int grad_layout, int T, int G, const void *const *feats,
                                  const int32_t *hw, int L, const float *loc, const float *w, void *const *grad_feats,
                                  float *grad_loc, int S, int N, int Q, int P, int C, int feat_layout, void *stream)
{
    return msmv_v2_bwd_impl("rac_msmv_v2_bwd_ex", grad_out, grad_layout, T, G, feats, hw, L, loc, w, grad_feats, grad_loc, S, N,
                            Q, P, C, feat_layout, stream);
}

extern "C" int rac_msmv_v2_bwd(const float *grad_out, const void *const *feats, const int32_t *hw, int L, const float *loc,
                               const float *w, void *const *grad_feats, float *grad_loc, int S, int N, int Q, int P, int C,
                               int feat_layout, void *stream)
{
    return msmv_v2_bwd_impl("rac_msmv_v2_bwd", grad_out, RAC_OUT_SQCP, 1, 1, feats, hw, L, loc, w, grad_feats, grad_loc, S, N, Q,
                            P, C, feat_layout, stream);
}
