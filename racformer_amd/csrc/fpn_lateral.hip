// fpn_lateral.hip -- the lateral 1x1 convolution of the image necks with the top-down merge (mmdet FPN.lateral_convs /
// the in-tree CustomFPN, models/necks/fpn.py:159-176) on the f16 matrix cores, straight from the channel-first backbone maps (gfx950):
//
//   out[n][co][p] = sum_ci W[co][ci] * x[n][ci][p] + bias[co] + (top ? top[n][co][src(p)] : 0)
//
// src(p) is the legacy 'nearest' rule of F.interpolate(top, size=(H, W)): per axis min((int)floorf(dst * scale), in - 1) with
// scale = (float)in / out, computed by the host in float32 (IEEE division, what torch computes) and multiplied here in float32.
//
// Arithmetic as in value_proj.hip: x * 2^e = hi + lo (two f16), W image [256][Cin/32][hi 32 | lo 32] from rac_gemm_split_pack_fwd,
// the three leading products lo*hi + hi*lo + hi*hi per K step in v_mfma_f32_16x16x32_f16, fp32 accumulate.  The activation scale
// 2^e is chosen PER PIXEL (max over the pixel's Cin channels -> largest value in [2^13, 2^14)): no pass over the maps for a global
// maximum, and a pixel of small magnitude keeps its 22 bits beside a large one.  Cin reaches 2048, so the pixel's maximum cannot be
// had from one stage as in value_proj: the workgroup walks its tile's channels twice -- once for the maxima, once for the products.
// The second walk finds the tile (Cin x 128 pixels x 4 B: 128 KB at Cin = 256, 1 MB at 2048) in L2 / the Infinity Cache.
//
// Workgroup = 256 threads = 4 waves, tile = 128 or 64 consecutive pixels of ONE image (template NJ = 8 / 4 MFMA tiles of 16 pixels; the
// launcher takes 128 where that gives every CU a workgroup) x all 256 output channels; K steps of 32 channels.  A wave owns 64 output
// channels x the tile's pixels = 4 x NJ MFMA tiles (128 / 64 accumulator registers); two workgroups share a CU (256 registers each), so
// one's first walk and epilogue run beside the other's products.  Per step the 32 x (16 NJ) fp32 block of x goes global -> registers ->
// (scale, split) -> LDS as [32 channels][16 NJ pixels] hi and lo images with the PIXEL contiguous, as in memory; the MFMA's B operand
// wants 8 consecutive channels of one pixel per lane, which ds_read_b64_tr_b16 delivers (a 16-lane group reads 4 channel rows x 16
// pixels, every lane receives its pixel's 4 channels; two reads per fragment).  Image layout and swizzle are those of linear_bwd.hip's
// wide operand (16-byte slot ch of row r at 16 (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))), masked to the row's slots: conflict-free
// transposed reads on 256-byte rows, see there).  Two LDS stages, the loads of step s + 1 in flight under the MFMAs of step s, one
// barrier per step.  The weights are the MFMA's A operand and come from their line image directly (a lane's fragment is 16 contiguous
// bytes of a line; 16 KB per step and workgroup, L2-resident), one step ahead in registers.
// Every load of x is unconditional: pixels past the image re-read its last ones and get the scale 0 (a select around a load became a
// branch and a full wait per load).  The first walk keeps four chunks' loads in flight.
// Epilogue: an accumulator tile has its pixel on the lane (column li) and four consecutive output channels in the lane's registers:
// per channel the 16 lanes li store 64 contiguous bytes and gather neighbouring pixels of the coarser level, the 16 gathers of a pixel
// tile issued together.  No atomics, nothing read back; the grid depends on the shapes alone.
// Any H, W: 16-byte loads when H*W % 4 == 0 and x is 16-byte aligned, 4-byte loads otherwise.
//
// The same kernel source is the convolution's data gradient (template DG, rac_fpn_lateral_dgrad at the end of this file):
//   dX[n][ci][p] = sum_co W[co][ci] * G[n][co][p]
// is this GEMM with K = 256, the merged gradient G as x (per-pixel scale as above), the line image of W^T (rac_linear_pack_wt) as the
// weights and Cin output channels in blocks of 256.  The rest of the backward is fpn_lateral_bwd.hip.
#include "split_f16.h"

#define FL_COUT 256

struct FpnLateralArgs {
    const float *x;      // [N][Cin][HW]
    const char *w;       // W image [256][Cin/32][hi 32 | lo 32] f16
    const float *bias;   // [256] or null
    const float *top;    // [N][256][hc*wc] or null
    float *out;          // [N][256][HW]
    float w_alpha, scale_h, scale_w;
    int HW, W, chunks, hc, wc, tiles_per_img;
    int cout, nblk;      // data gradient only: output channels (rows of the weight image that are stored), blocks of 256 of them
};

// NJ: 16-pixel MFMA tiles per workgroup (8: 128 pixels, 4: 64 pixels).  VEC: 16-byte loads (H*W % 4 == 0, x 16-byte aligned).
// HAS_TOP: the top-down term is gathered in the epilogue.
// DG: the data gradient of the same convolution (rac_fpn_lateral_dgrad): x is the merged gradient G [N][256][HW], the weight image that
// of W^T (a.cout = the forward's Cin rows, padded to whole blocks of 256), out = dX [N][a.cout][HW].  The grid carries the a.nblk
// blocks of 256 output channels innermost, so the workgroups that share a tile of G run together; channels past a.cout (a last block
// of fewer than 256) are computed on the padding rows and not stored.  No bias, no top.
template <int NJ, bool VEC, bool HAS_TOP, bool DG = false>
__global__ __launch_bounds__(256, 2) void fpn_lateral_kernel(const FpnLateralArgs a)
{
    static_assert(!(DG && HAS_TOP), "the data gradient has no top-down term");
    constexpr int TP = 16 * NJ;            // pixels per workgroup
    constexpr int RB = 2 * TP;             // bytes per LDS row (one channel's TP pixels, f16)
    constexpr int HALF = 32 * RB;          // one of hi / lo of a stage
    constexpr int STAGE = 2 * HALF;
    constexpr int TPR = 2 * NJ;            // staging threads per channel row (8 pixels each) = 16-byte slots per LDS row
    constexpr int RP = 256 / TPR;          // channel rows per staging pass
    constexpr int NI = 32 / RP;            // staging passes (items per thread) per step
    __shared__ __attribute__((aligned(16))) char fl_lds[2 * STAGE];
    __shared__ __attribute__((aligned(16))) float fl_unscale[TP], fl_scale[TP];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int HW = a.HW, chunks = a.chunks;
    const int bid = DG ? blockIdx.x / a.nblk : blockIdx.x;
    const int cbase = DG ? FL_COUT * (blockIdx.x - bid * a.nblk) : 0;      // first output channel of this workgroup
    const int n = bid / a.tiles_per_img, tile = bid - n * a.tiles_per_img;
    const int p0 = tile * TP;
    const float *__restrict__ xn = a.x + (size_t)n * chunks * 32 * HW;

    // staging role: item j < NI = channel row r = tid / TPR + RP j of the step, pixels p0 + 8 (tid % TPR) .. + 7: LDS slot tid % TPR.
    // Pixels past the image re-read its last ones (a valid address, no predicate: a select here becomes a branch around every load)
    // and get the scale 0 below: their columns of the product are zero and are not stored.
    const int s_rb = tid / TPR, s_ch = tid % TPR, s_p = p0 + 8 * s_ch;
    int s_off[VEC ? 2 : 8];
#pragma unroll
    for (int e = 0; e < (VEC ? 2 : 8); ++e)
        s_off[e] = VEC ? min(s_p + 4 * e, HW - 4) : min(s_p + e, HW - 1);
    auto gload = [&](int c, rac_f4v *rx) {
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const float *row = xn + (size_t)(c * 32 + s_rb + RP * j) * HW;
            if (VEC) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    rx[2 * j + h] = *reinterpret_cast<const rac_f4v *>(row + s_off[h]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    rx[2 * j + (e >> 2)][e & 3] = row[s_off[e]];
            }
        }
    };

    // ---- first walk: per-pixel maximum over all channels.  This thread's 8 pixels over its NI rows of every chunk, four chunks'
    // loads in flight at a time (past the end the last chunk again: unconditional code), then the RP row classes through LDS.
    float mx[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
        mx[e] = 0.f;
    for (int c = 0; c < chunks; c += 4) {
        rac_f4v r4[4][2 * NI];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            gload(min(c + u, chunks - 1), r4[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < NI; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    mx[e] = fmaxf(mx[e], fabsf(r4[u][2 * j + (e >> 2)][e & 3]));
    }
    {
        float *red = reinterpret_cast<float *>(fl_lds);      // [RP row classes][TP pixels]
#pragma unroll
        for (int e = 0; e < 8; ++e)
            red[s_rb * TP + 8 * s_ch + e] = mx[e];
        __syncthreads();
        // the first row class combines them and writes the tile's scales: 2^(13 - e) with e = floor(log2(max)), exponent arithmetic only
        // (max = 0 / denormal / inf: clamped exponents) as value_proj.hip, 0 for pixels past the image; and the epilogue's 2^(e - 13) w_alpha.
        // (In LDS, re-read by every lstore: eight registers fewer across the product loop, whose budget is 256 for two workgroups per CU.)
        if (s_rb == 0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float m = red[8 * s_ch + e];
#pragma unroll 4
                for (int g = 1; g < RP; ++g)
                    m = fmaxf(m, red[g * TP + 8 * s_ch + e]);
                int eb = (int)((__float_as_uint(m) >> 23) & 255u);
                eb = eb < 14 ? 14 : (eb > 254 ? 254 : eb);
                fl_scale[8 * s_ch + e] = s_p + e < HW ? __uint_as_float((unsigned)(267 - eb) << 23) : 0.f;
                fl_unscale[8 * s_ch + e] = a.w_alpha * __uint_as_float((unsigned)(eb - 13) << 23);
            }
        }
    }
    __syncthreads();     // the scales are in place and the maxima read: the stages may be written

    rac_f4v rx[2 * NI];
    auto lstore = [&](int buf) {
        char *S = fl_lds + buf * STAGE;
        const rac_f4v sc0 = *reinterpret_cast<const rac_f4v *>(fl_scale + 8 * s_ch), sc1 = *reinterpret_cast<const rac_f4v *>(fl_scale + 8 * s_ch + 4);
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int r = s_rb + RP * j;
            rac_h8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float s = rx[2 * j + (e >> 2)][e & 3] * (e < 4 ? sc0[e & 3] : sc1[e & 3]);
                hi[e] = (_Float16)s;
                lo[e] = (_Float16)(s - (float)hi[e]);
            }
            char *d = S + RB * r + 16 * (s_ch ^ (rac_tr_swz(r) & (TPR - 1)));
            *reinterpret_cast<rac_h8 *>(d) = hi;
            *reinterpret_cast<rac_h8 *>(d + HALF) = lo;
        }
    };

    // weight fragments of this wave's 64 output channels: tile i = rows 64 wave + 16 i + li, chunk lk of the line's hi / lo half
    const char *__restrict__ wrow = a.w + (size_t)(cbase + 64 * wave + li) * chunks * 128 + lk * 16;
    const size_t wstep = (size_t)16 * chunks * 128;
    rac_h8 wh[4], wl[4], nwh[4], nwl[4];
    auto wload = [&](int c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            nwh[i] = *reinterpret_cast<const rac_h8 *>(wrow + i * wstep + (size_t)c * 128);
            nwl[i] = *reinterpret_cast<const rac_h8 *>(wrow + i * wstep + (size_t)c * 128 + 64);
        }
    };

    // transposed-read addresses: lane 4 q + p of a 16-lane group supplies channel row q, pixels 4 p .. 4 p + 3 of the tile's 16, i.e.
    // 16-byte slot (p >> 1) of the tile's two, byte 8 (p & 1) in it.  Block blk of lane group lk holds rows 8 lk + 4 blk + q.
    // Tile j's slots are 2 j and 2 j + 1, and (2 j + b) ^ sw = (2 j) ^ (b ^ sw): tile j is tile 0's address ^ (32 j) -- two address
    // registers instead of 2 NJ.
    int xa[2];
    {
        const int q = li >> 2, p = li & 3;
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int r = 8 * lk + 4 * blk + q, sw = rac_tr_swz(r) & (TPR - 1);
            xa[blk] = RB * r + 16 * ((p >> 1) ^ sw) + 8 * (p & 1);
        }
    }

    rac_f4v acc[4][NJ];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
            acc[i][j] = (rac_f4v){0.f, 0.f, 0.f, 0.f};

    // ---- second walk: the products.  (Uniform control flow over the workgroup: the transposed reads need every lane active.)
    gload(0, rx);
    wload(0);
    lstore(0);
    __syncthreads();
    for (int c = 0; c < chunks; ++c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            wh[i] = nwh[i];
            wl[i] = nwl[i];
        }
        const int cn = c + 1 < chunks ? c + 1 : c;      // (past the end the last step is re-fetched: unconditional code)
        gload(cn, rx);
        wload(cn);
        // (nothing may move across these lines: without them hipcc hoists the conversion of step c + 1 -- and with it the wait for the
        //  loads just issued -- in front of the MFMAs)
        __builtin_amdgcn_sched_barrier(0);
        const char *S = fl_lds + (c & 1) * STAGE;
        int xa0 = xa[0], xa1 = xa[1];
        asm volatile("" : "+v"(xa0), "+v"(xa1));     // (per step: otherwise the 2 NJ tile addresses are hoisted out of the loop -- and spilled)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const rac_h8 xh = rac_tr_frag(S, xa0 ^ (32 * j), xa1 ^ (32 * j));
            const rac_h8 xl = rac_tr_frag(S + HALF, xa0 ^ (32 * j), xa1 ^ (32 * j));
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[i], xh, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[i], xl, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[i], xh, acc[i][j], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        lstore((c + 1) & 1);        // the stage read during step c - 1: free since the barrier that ended it
        __syncthreads();
    }

    // ---- epilogue.  Accumulator tile (i, j): rows 4 lk + r = output channels (the MFMA's A operand), column li = pixel: per channel
    // the 16 lanes li store 64 contiguous bytes, and gather at most 16 neighbouring pixels of the coarser level.  The 16 gathers of a
    // pixel tile are issued together, ahead of its stores.
    float *__restrict__ on = a.out + (size_t)n * (DG ? a.cout : FL_COUT) * HW + (size_t)cbase * HW;
    const int tplane = a.hc * a.wc;
    const float *__restrict__ tn = HAS_TOP ? a.top + (size_t)n * FL_COUT * tplane : nullptr;
    rac_f4v bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        bv[i] = a.bias ? *reinterpret_cast<const rac_f4v *>(a.bias + 64 * wave + 16 * i + 4 * lk) : (rac_f4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int pl = 16 * j + li, p = p0 + pl;
        const bool live = p < HW;
        const int pc = live ? p : HW - 1;
        const float us = fl_unscale[pl];
        float tv[4][4];
        if (HAS_TOP) {
            const int h = pc / a.W, w = pc - h * a.W;
            const int sh = min((int)floorf((float)h * a.scale_h), a.hc - 1);
            const int sw = min((int)floorf((float)w * a.scale_w), a.wc - 1);
            const float *tp = tn + (size_t)(64 * wave + 4 * lk) * tplane + sh * a.wc + sw;
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    tv[i][r] = tp[(size_t)(16 * i + r) * tplane];
        }
        if (live) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (DG && cbase + 64 * wave + 16 * i >= a.cout)      // (wave-uniform: a.cout is a multiple of 32)
                    continue;
                const rac_f4v v = __builtin_elementwise_fma(acc[i][j], (rac_f4v){us, us, us, us}, bv[i]);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    on[(size_t)(64 * wave + 16 * i + 4 * lk + r) * HW + p] = HAS_TOP ? v[r] + tv[i][r] : v[r];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" int rac_fpn_lateral_fwd(const float *x, const void *w_image, float w_alpha, const float *bias, const float *top, float *out,
                                   int N, int Cin, int H, int W, int top_h, int top_w, int Cout, void *stream)
{
    const char *what = "rac_fpn_lateral_fwd";
    RAC_CHECK_ARG(Cout == FL_COUT, "%s: built for %d output channels (got %d)", what, FL_COUT, Cout);
    RAC_CHECK_ARG(Cin >= 32 && Cin % 32 == 0, "%s: Cin=%d (a multiple of 32)", what, Cin);
    RAC_CHECK_ARG(N >= 0 && H >= 1 && W >= 1 && (long)H * W < (1l << 30), "%s: N=%d H=%d W=%d", what, N, H, W);
    RAC_CHECK_ARG(!top || (top_h >= 1 && top_w >= 1 && top_h <= H && top_w <= W),
                  "%s: top %dx%d must be at least 1x1 and no larger than the output %dx%d", what, top_h, top_w, H, W);
    if (N == 0)
        return 0;
    RAC_CHECK_ARG(x && w_image && out, "%s: null pointer", what);
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(w_image) | reinterpret_cast<uintptr_t>(bias)) & 15) == 0,
                  "%s: w_image / bias must be 16-byte aligned", what);
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(top)) & 3) == 0,
                  "%s: x / top / out must be 4-byte aligned", what);
    // 128-pixel tiles where they give every CU a workgroup (256 tiles), 64-pixel tiles below (twice the weight traffic per pixel, but
    // more workgroups for the deep, small levels): a function of the shapes alone
    const int HW = H * W;
    const bool wide = (long)N * ((HW + 127) / 128) >= 256;
    const int tp = wide ? 128 : 64, tiles = (HW + tp - 1) / tp;
    RAC_CHECK_ARG((long)N * tiles < (1l << 31), "%s: %ld workgroups", what, (long)N * tiles);
    FpnLateralArgs a;
    a.x = x; a.w = reinterpret_cast<const char *>(w_image); a.bias = bias; a.top = top; a.out = out;
    a.w_alpha = w_alpha;
    a.scale_h = top ? (float)top_h / (float)H : 1.f;
    a.scale_w = top ? (float)top_w / (float)W : 1.f;
    a.HW = HW; a.W = W; a.chunks = Cin / 32; a.hc = top ? top_h : 1; a.wc = top ? top_w : 1; a.tiles_per_img = tiles;
    a.cout = FL_COUT; a.nblk = 1;
    const bool vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
    const dim3 grid((unsigned)(N * tiles));
    hipStream_t st = (hipStream_t)stream;
#define FL_GO(NJ_)                                                                                              \
    do {                                                                                                        \
        if (vec && top) hipLaunchKernelGGL((fpn_lateral_kernel<NJ_, true, true>), grid, dim3(256), 0, st, a);   \
        else if (vec) hipLaunchKernelGGL((fpn_lateral_kernel<NJ_, true, false>), grid, dim3(256), 0, st, a);    \
        else if (top) hipLaunchKernelGGL((fpn_lateral_kernel<NJ_, false, true>), grid, dim3(256), 0, st, a);    \
        else hipLaunchKernelGGL((fpn_lateral_kernel<NJ_, false, false>), grid, dim3(256), 0, st, a);            \
    } while (0)
    if (wide) FL_GO(8);
    else FL_GO(4);
#undef FL_GO
    return rac_launch_status(what);
}

// dX[n][ci][p] = sum_co W[co][ci] * G[n][co][p]: the forward's GEMM with K = 256 and Cin output channels, on the image of W^T.
extern "C" int rac_fpn_lateral_dgrad(const float *g, const void *wt_image, float w_alpha, float *dx, int N, int Cin, int H, int W,
                                     int Cout, void *stream)
{
    const char *what = "rac_fpn_lateral_dgrad";
    RAC_CHECK_ARG(Cout == FL_COUT, "%s: built for %d output channels (got %d)", what, FL_COUT, Cout);
    RAC_CHECK_ARG(Cin >= 32 && Cin % 32 == 0 && Cin <= 2048, "%s: Cin=%d (a multiple of 32 from 32 to 2048)", what, Cin);
    RAC_CHECK_ARG(N >= 0 && H >= 1 && W >= 1 && (long)H * W < (1l << 30), "%s: N=%d H=%d W=%d", what, N, H, W);
    if (N == 0)
        return 0;
    RAC_CHECK_ARG(g && wt_image && dx, "%s: null pointer", what);
    RAC_CHECK_ARG((reinterpret_cast<uintptr_t>(wt_image) & 15) == 0, "%s: wt_image must be 16-byte aligned", what);
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(dx)) & 3) == 0, "%s: g / dx must be 4-byte aligned", what);
    const int HW = H * W, nblk = (Cin + FL_COUT - 1) / FL_COUT;
    const bool wide = (long)N * ((HW + 127) / 128) * nblk >= 256;      // the forward's rule, over all the workgroups
    const int tp = wide ? 128 : 64, tiles = (HW + tp - 1) / tp;
    RAC_CHECK_ARG((long)N * tiles * nblk < (1l << 31), "%s: %ld workgroups", what, (long)N * tiles * nblk);
    FpnLateralArgs a;
    a.x = g; a.w = reinterpret_cast<const char *>(wt_image); a.bias = nullptr; a.top = nullptr; a.out = dx;
    a.w_alpha = w_alpha; a.scale_h = 1.f; a.scale_w = 1.f;
    a.HW = HW; a.W = W; a.chunks = FL_COUT / 32; a.hc = 1; a.wc = 1; a.tiles_per_img = tiles;
    a.cout = Cin; a.nblk = nblk;
    const bool vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(g) & 15) == 0;
    const dim3 grid((unsigned)(N * tiles * nblk));
    hipStream_t st = (hipStream_t)stream;
    if (wide && vec) hipLaunchKernelGGL((fpn_lateral_kernel<8, true, false, true>), grid, dim3(256), 0, st, a);
    else if (wide) hipLaunchKernelGGL((fpn_lateral_kernel<8, false, false, true>), grid, dim3(256), 0, st, a);
    else if (vec) hipLaunchKernelGGL((fpn_lateral_kernel<4, true, false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((fpn_lateral_kernel<4, false, false, true>), grid, dim3(256), 0, st, a);
    return rac_launch_status(what);
}
