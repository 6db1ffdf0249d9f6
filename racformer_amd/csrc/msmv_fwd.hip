// msmv_fwd.hip -- multi-scale multi-view sampling, forward, for gfx950 (MI355X).
//
// Replaces the reference's ms_deformable_im2col_gpu_kernel_{c45,c2345,c23456}
// (models/csrc/msmv_sampling/msmv_sampling_forward.cu:75-334) behind rac_msmv_fwd.
// Semantics (same as the reference kernel, :105-157 and :27-73): per point, view =
// round(loc_v*(N-1)); per level h_im = v*(H-1), w_im = u*(W-1) (align_corners=True), level
// skipped unless h_im>-1 && w_im>-1 && h_im<H && w_im<W; 4 bilinear taps, each bounds-checked,
// zero padding; levels accumulated in order c2..c5 with their scale weight.
//
// CDNA4 mapping (not the reference's thread-per-channel scheme):
//  * C=64 fast path: a 16-lane group owns one sampling point; each lane holds 4 adjacent
//    channels, so every tap is one 16-byte load per lane and one wave-instruction fetches four
//    256-byte pixel rows (1 KiB).  A wave64 walks the P points of one (slot, query) row four at
//    a time; all 4 levels x 4 taps = 16 independent loads are in flight per lane before the
//    first FMA.  No cross-lane reduction is needed: the reduction over levels/taps is in-register.
//  * the bilinear footprint of a point is computed ONCE (one thread per point, into an LDS tap table: four byte
//    offsets + four weights per level), not by each of the 16 lanes that gather it; the taps are buffer-descriptor
//    loads whose range check zero-fills taps outside the map (no branches), the accumulation is packed FMAs.
//  * block -> (slot, query block) mapping is XCD-aware: blocks b and b+8 share an XCD (and its
//    4 MiB L2), so XCD x walks slots x, x+8, ... and the 32 CUs of one XCD work on the same
//    slot's 23 MB pyramid at the same time, neighbouring queries (adjacent rays) together.
//  * RAC_OUT_BQGTPC writes the consumer layout directly: each 16-lane group stores one 256-byte
//    pixel row, 1 KiB contiguous per wave-instruction (the reference's P-minor layout needs
//    48-byte-strided 4-byte stores and a separate 88 MB permute afterwards).
#include "gather_device.h"

#define MSMV_ROWS 8 /* (slot,query) rows per 256-thread workgroup: two per wave */

template <typename FT, int L, bool OUT_CL>
__global__ __launch_bounds__(256, (L <= 4 ? 4 : 3)) void msmv_fwd_c64_kernel(const MsmvArgs a)
{
    extern __shared__ float smem[];
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63, sub = lane >> 4, c4 = lane & 15;
    const int P = a.P;

    const int xcd = blockIdx.x & 7;
    const int j = blockIdx.x >> 3;
    const int s = xcd + 8 * (j / a.blocks_per_slot);
    if (s >= a.S)
        return;
    const int q0 = (j % a.blocks_per_slot) * MSMV_ROWS;
    const int nrows = min(MSMV_ROWS, a.Q - q0);

    // tap table [L][rows*P][8]: per point and level the 4 tap byte offsets into the level's buffer (RAC_TAP_OUTSIDE =
    // outside the map) and the 4 bilinear weights with the level's scale weight folded in -- one thread per point builds it
    // from the op's loc / weight rows, instead of each of the 16 lanes that gather the point
    float *stab = smem;
    const int lstride = MSMV_ROWS * P * 8;
    const size_t row0 = (size_t)s * a.Q + q0;
    for (int i = tid; i < nrows * P; i += 256) {
#pragma clang fp contract(off)   // (the weight products rounded one by one as well, as the reference's statements read)
        const float *lp = a.loc + (row0 * P + i) * 3;
        const float *wp = a.w + (row0 * P + i) * L;
        const float lu = lp[0], lv = lp[1];
        const int view = rac_msmv_view(lp[2], a.N);
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const int H = a.H[l], W = a.W[l];
            const RacFootprint f = rac_footprint(lv * (float)(H - 1), lu * (float)(W - 1), H, W);
            const int h_low = f.h_low, w_low = f.w_low, h_high = h_low + 1, w_high = w_low + 1;
            const unsigned pix_bytes = (unsigned)(64 * sizeof(FT));
            const unsigned mbase = (unsigned)view * (unsigned)(H * W) * pix_bytes;   // camera's map inside the slot's block of the level
            rac_u4 off;
            off.x = f.ok[0] ? mbase + (unsigned)(h_low * W + w_low) * pix_bytes : RAC_TAP_OUTSIDE;
            off.y = f.ok[1] ? mbase + (unsigned)(h_low * W + w_high) * pix_bytes : RAC_TAP_OUTSIDE;
            off.z = f.ok[2] ? mbase + (unsigned)(h_high * W + w_low) * pix_bytes : RAC_TAP_OUTSIDE;
            off.w = f.ok[3] ? mbase + (unsigned)(h_high * W + w_high) * pix_bytes : RAC_TAP_OUTSIDE;
            const float wl = wp[l];
            float *e = stab + l * lstride + i * 8;
            *reinterpret_cast<rac_u4 *>(e) = off;
            *reinterpret_cast<rac_f4 *>(e + 4) = (rac_f4){f.hh * f.hw * wl, f.hh * f.lw * wl, f.lh * f.hw * wl, f.lh * f.lw * wl};
        }
    }
    __syncthreads();
    // (the slot index through readfirstlane: the descriptor base then is scalar arithmetic -- left to itself hipcc computes it in
    //  vector registers and wraps every buffer load in a waterfall loop over a descriptor it can no longer prove uniform: +6 us)
    const int s_uni = __builtin_amdgcn_readfirstlane(s);
    __amdgpu_buffer_rsrc_t rsrc[L];
#pragma unroll
    for (int l = 0; l < L; ++l)
        // (one descriptor per level over THIS SLOT's N maps: offsets are relative to the slot, so only a slot's bytes -- not the whole
        //  level's, B * T * G slots -- have to stay below the 31-bit tap offsets)
        rsrc[l] = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(reinterpret_cast<const char *>(a.feat[l]) + (size_t)s_uni * a.feat_bytes[l]), 0,
                                                    a.feat_bytes[l], 0x00020000);
    const unsigned lane_off = (unsigned)(c4 * 4 * sizeof(FT));
    // wave w gathers rows w, w+4 of the workgroup; per tap: one add for the lane's channel offset, one buffer load, two
    // packed FMAs; 16 taps (4 levels x 4) in flight per lane
    for (int row = wave; row < nrows; row += 4) {
        const int q = q0 + row;
        const size_t out_row = msmv_out_index(a, OUT_CL, s, q, 0).base;  // element offset of this row's output block
        for (int p0 = 0; p0 < P; p0 += 4) {
            const int p = p0 + sub;
            const bool act = p < P;
            const float *e = stab + (row * P + (act ? p : P - 1)) * 8;
            rac_f4 v[L][4], tw[L];
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const rac_u4 o = *reinterpret_cast<const rac_u4 *>(e + l * lstride);
                tw[l] = *reinterpret_cast<const rac_f4 *>(e + l * lstride + 4);
                if (l == 0) {   // level 0 through the non-temporal tap; measured on SURVEY 8d's uniform-stress set: 122 -> 112 us per launch (60 -> 65 % of the roofline)
                    v[l][0] = rac_tap<FT, 2>(rsrc[l], o.x + lane_off);
                    v[l][1] = rac_tap<FT, 2>(rsrc[l], o.y + lane_off);
                    v[l][2] = rac_tap<FT, 2>(rsrc[l], o.z + lane_off);
                    v[l][3] = rac_tap<FT, 2>(rsrc[l], o.w + lane_off);
                } else {
                    v[l][0] = rac_tap<FT>(rsrc[l], o.x + lane_off);
                    v[l][1] = rac_tap<FT>(rsrc[l], o.y + lane_off);
                    v[l][2] = rac_tap<FT>(rsrc[l], o.z + lane_off);
                    v[l][3] = rac_tap<FT>(rsrc[l], o.w + lane_off);
                }
            }
#if defined(RAC_DIAGNOSTIC_BUILD) && defined(RAC_GATHER_LOADS_FIRST)
            __builtin_amdgcn_sched_barrier(0);   // diagnostic (tools/race_victims.py): every tap load is issued before the first FMA
#endif
            rac_acc4 acc4 = rac_acc4_zero();
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const float w4[4] = {tw[l].x, tw[l].y, tw[l].z, tw[l].w};
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    rac_tap_fma(acc4, v[l][c].x, v[l][c].y, v[l][c].z, v[l][c].w, w4[c]);
                }
            }
            if (act) {
                rac_f4 r;
                rac_acc4_get(acc4, r.x, r.y, r.z, r.w);
                if (OUT_CL) {
                    *reinterpret_cast<rac_f4 *>(a.out + out_row + (size_t)p * 64 + c4 * 4) = r;
                } else {
                    float *o = a.out + out_row + (size_t)(c4 * 4) * P + p;
                    o[0] = r.x;
                    o[(size_t)P] = r.y;
                    o[(size_t)2 * P] = r.z;
                    o[(size_t)3 * P] = r.w;
                }
            }
        }
    }
}

// Any C / any L<=8: one thread per (row, point, channel), channel fastest (coalesced taps).
template <typename FT>
__global__ __launch_bounds__(256) void msmv_fwd_generic_kernel(const MsmvArgs a)
{
    const long total = (long)a.S * a.Q * a.P * a.C;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long)gridDim.x * blockDim.x) {
        const int c = (int)(idx % a.C);
        const long rp = idx / a.C;
        const int p = (int)(rp % a.P);
        const long r = rp / a.P;
        const int s = (int)(r / a.Q), q = (int)(r % a.Q);
        const float *lp = a.loc + rp * 3;
        const float *wp = a.w + rp * a.L;
        const float lu = lp[0], lv = lp[1];
        const int view = rac_msmv_view(lp[2], a.N);
        float acc = 0.f;
        for (int l = 0; l < a.L; ++l) {
            const int H = a.H[l], W = a.W[l];
            const RacFootprint f = rac_footprint(lv * (float)(H - 1), lu * (float)(W - 1), H, W);
            if (!f.in)
                continue;
            const int h_low = f.h_low, w_low = f.w_low, h_high = h_low + 1, w_high = w_low + 1;
            const FT *base = (const FT *)a.feat[l] + ((size_t)s * a.N + view) * H * W * a.C + c;
            float v1 = 0.f, v2 = 0.f, v3 = 0.f, v4 = 0.f;
            if (f.ok[0]) v1 = rac_ld1(base + ((size_t)h_low * W + w_low) * a.C);
            if (f.ok[1]) v2 = rac_ld1(base + ((size_t)h_low * W + w_high) * a.C);
            if (f.ok[2]) v3 = rac_ld1(base + ((size_t)h_high * W + w_low) * a.C);
            if (f.ok[3]) v4 = rac_ld1(base + ((size_t)h_high * W + w_high) * a.C);
            acc += (f.hh * f.hw * v1 + f.hh * f.lw * v2 + f.lh * f.hw * v3 + f.lh * f.lw * v4) * wp[l];
        }
        a.out[msmv_out_index(a, a.T > 0, s, q, p, c).base] = acc;
    }
}

template <typename FT, bool OUT_CL>
static int launch_c64(const MsmvArgs &a, hipStream_t st)
{
    const int nb = 8 * ((a.S + 7) / 8) * a.blocks_per_slot;
    const size_t lds = (size_t)MSMV_ROWS * a.P * 8 * a.L * sizeof(float);
    switch (a.L) {
    case 2: hipLaunchKernelGGL((msmv_fwd_c64_kernel<FT, 2, OUT_CL>), dim3(nb), dim3(256), lds, st, a); break;
    case 4: hipLaunchKernelGGL((msmv_fwd_c64_kernel<FT, 4, OUT_CL>), dim3(nb), dim3(256), lds, st, a); break;
    case 5: hipLaunchKernelGGL((msmv_fwd_c64_kernel<FT, 5, OUT_CL>), dim3(nb), dim3(256), lds, st, a); break;
    default: return 1;
    }
    return 0;
}

extern "C" int rac_msmv_fwd(const void *const *feats, const int32_t *hw, int L, const float *loc,
                            const float *w, float *out, int S, int N, int Q, int P, int C, int dtype,
                            int out_layout, int T, int G, void *stream)
{
    MsmvArgs a;
    const int rc = msmv_fill_args(a, MSMV_FWD, "rac_msmv_fwd", out_layout, T, G, feats, nullptr, hw, L, loc, w, out != nullptr,
                                  S, N, Q, P, C, dtype, RAC_FEAT_CL);
    if (rc || a.S == 0)
        return rc;
    bool small_maps = true;
    for (int l = 0; l < L; ++l) {
        const size_t bytes = (size_t)N * a.H[l] * a.W[l] * C * (dtype == RAC_F32 ? 4 : 2);        // one slot's maps
        a.feat_bytes[l] = bytes < (size_t)RAC_TAP_OUTSIDE ? (unsigned)bytes : 0u;    // 0: too large for the 31-bit tap offsets
        small_maps = small_maps && a.feat_bytes[l] != 0;
    }
    a.out = out;
    a.blocks_per_slot = (Q + MSMV_ROWS - 1) / MSMV_ROWS;
    hipStream_t st = (hipStream_t)stream;
    int fell_through = 1;
    if (C == 64 && (L == 2 || L == 4 || L == 5) && small_maps && (size_t)MSMV_ROWS * P * 8 * L * sizeof(float) <= 64 * 1024) {
        if (dtype == RAC_F32)
            fell_through = out_layout == RAC_OUT_BQGTPC ? launch_c64<float, true>(a, st) : launch_c64<float, false>(a, st);
        else
            fell_through = out_layout == RAC_OUT_BQGTPC ? launch_c64<unsigned short, true>(a, st)
                                                        : launch_c64<unsigned short, false>(a, st);
    }
    if (fell_through) {
        const long total = (long)S * Q * P * C;
        const int nb = (int)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
        if (dtype == RAC_F32)
            hipLaunchKernelGGL(msmv_fwd_generic_kernel<float>, dim3(nb), dim3(256), 0, st, a);
        else
            hipLaunchKernelGGL(msmv_fwd_generic_kernel<unsigned short>, dim3(nb), dim3(256), 0, st, a);
    }
    return rac_launch_status("rac_msmv_fwd");
}
