// conv3x3_bwd.hip -- the backward of the temporal-fusion convolution (conv3x3.hip: 3x3, stride 1, pad 1, Cin -> 256) on the
// f16 matrix cores with the forward's arithmetic: operands split hi + lo (two f16, 22 significant bits), the three leading
// products hi*hi + hi*lo + lo*hi accumulated in fp32 by v_mfma_f32_16x16x32_f16 (gfx950).
//
// Data gradient: dX = conv3x3(dY, W') with W'[ci][co][ky][kx] = W[co][ci][2-ky][2-kx] IS the forward kernel (rac_conv3x3_fwd) on an
// activation image of dY and a weight image packed from W' by the host; this file adds only the pack of a channel-LAST fp32 source
// (autograd hands dY over in the layout the forward wrote) into that image.
//
// Weight gradient: dW[co][ci][ky][kx] = sum_{n,h,w} dY[n,co,h,w] X[n,ci,h+ky-1,w+kx-1], a GEMM with M = 256 (co), N = 9 Cin (tap, ci)
// and K = N H W (pixels).  Both operands sum over the PIXEL index while the activation images keep the channels in the fast
// dimension, so the MFMA fragments (8 consecutive k per lane) are read from LDS with ds_read_b64_tr_b16: a 16-lane group reads 4
// pixel rows x 16 channels and every lane receives its channel's 4 pixels; two such reads make one fragment.  dY and X fragments
// use the same pixel <-> k assignment (lane group lk, element 4 blk + q <-> pixel 8 lk + 4 blk + q of the step), which is all
// the product needs.
//   Workgroup = 256 threads = 4 waves, output tile = 128 co x 32 ci (one chunk) x 9 taps; a wave owns 32 co: 2 x 2 x 9
//   accumulator tiles (144 registers).  K-step = up to 32 consecutive pixels of ONE image row (row h, columns w0 .. w0+31; columns
//   past W are staged as zeros of dY).  Staged per step: dY [32 px][128 co] hi and lo (16 KB), and the halo of X that serves all
//   nine taps -- padded rows h .. h+2, padded columns w0 .. w0+33 of the chunk, [102 px][32 ci] hi and lo (12.75 KB, in 16 KB of LDS); the image's
//   zero border is the convolution's padding, so no tap is predicated.  Two LDS stages (64 KB: two workgroups per CU), global ->
//   registers -> LDS with the loads of step s+1 in flight under the MFMAs of step s, one barrier per step.
//   LDS images (16-byte slots, the swizzles make every transposed read conflict-free under the 64-bank rule):
//     dY  256-byte rows, slot ch (0..15) of row r at 256 r + 16 (ch ^ (((r & 3) << 2) | ((r >> 2) & 3)))
//     X   64-byte rows,  slot s (0..3)  of row r at  64 r + 16 (s ^ (2 ((r >> 3) & 1)))
//   Why conflict-free: a 32-lane half of a transposed read is two 16-lane groups (lk, lk + 1), each 4 rows x 32 bytes, rows
//   r .. r+3 and r+8 .. r+11, and the 64 banks are one 256-byte window.  X: rows r .. r+3 lie 64 bytes apart (four distinct
//   quarters of the window), and r -> r+8 flips bit 3 of the row, i.e. the 32-byte half of the quarter.  dY: rows are whole
//   windows; the XOR puts (r & 3) into bits 2-3 of the slot and ((r >> 2) & 3) -- whose bit 1 is what r -> r+8 flips -- into bits
//   0-1, so the 16 (row, 16-byte slot) pairs of a half take 16 distinct slots.  All addresses are multiples of 8.
//   K split: the N*H image rows are dealt out in `k_splits` contiguous ranges; workgroup (range p, tile) writes its partial sums
//   to workspace[p][tap][co][Cin], and a second launch adds the ranges in ascending p -- a fixed order, no float atomics: two runs
//   give the same bits.
#include "split_f16.h"

#define CB_COUT 256
#define CB_TM 128          /* co per workgroup */
#define CB_KP 32           /* pixels per K-step */
#define CB_XCOLS (CB_KP + 2)
#define CB_XROWS (3 * CB_XCOLS)                    /* 102 halo pixels */
#define CB_XROWS_LDS 128                           /* LDS rows: the staging pass writes 1024 slots unconditionally */
#define CB_G_BYTES (CB_KP * CB_TM * 2)             /* 8192: one of hi / lo of the dY tile */
#define CB_X_BYTES (CB_XROWS_LDS * 64)             /* 8192: one of hi / lo of the X halo */
#define CB_STAGE_BYTES (2 * CB_G_BYTES + 2 * CB_X_BYTES)   /* 32768 */

// ------------------------------------------------------------------------------------------------ pack, channel-last source
// [N][H][W][C] f32 -> channel chunks chunk0.. of the activation image (interior pixels; the border stays zero).  One thread = one
// pixel's 8 consecutive channels: 32 bytes in, 16 bytes of hi and 16 bytes of lo out.
__global__ __launch_bounds__(256) void conv_pack_cl_kernel(const float *__restrict__ src, const float *__restrict__ amax,
                                                           _Float16 *__restrict__ dst, long total, int C, int H, int W, int chunks_total,
                                                           int chunk0)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total)
        return;
    const int c8n = C >> 3;
    const long pix = i / c8n;
    const int c8 = (int)(i - pix * c8n);
    const int w = (int)(pix % W), h = (int)((pix / W) % H);
    const long n = pix / ((long)W * H);
    const float scale = rac_act_scale(*amax);
    const rac_f4 v0 = rac_ld4(src + i * 8), v1 = rac_ld4(src + i * 8 + 4);
    const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    rac_h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float s = v[j] * scale;
        hi[j] = (_Float16)s;
        lo[j] = (_Float16)(s - (float)hi[j]);
    }
    const size_t p = ((size_t)n * (H + 2) + h + 1) * (W + 2) + w + 1;
    _Float16 *o = dst + (p * chunks_total + chunk0 + (c8 >> 2)) * 64 + (c8 & 3) * 8;
    *reinterpret_cast<rac_h8 *>(o) = hi;
    *reinterpret_cast<rac_h8 *>(o + 32) = lo;
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct WgradArgs {
    const uint4 *xs;    // image of X  [N][H+2][W+2][chunks][2][32] f16
    const uint4 *gs;    // image of dY [N][H+2][W+2][8][2][32] f16
    float *ws;          // partial sums [k_splits][9][256][Cin]
    int N, H, W, chunks, k_splits;
};

__global__ __launch_bounds__(256, 2) void conv3x3_wgrad_f16x3_kernel(const WgradArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char cb_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int H = a.H, W = a.W, Wp = W + 2, chunks = a.chunks;
    const int chunk = blockIdx.x % chunks, ct = (blockIdx.x / chunks) & 1, part = blockIdx.x / (2 * chunks);
    const int rows_total = a.N * H, rows_per = (rows_total + a.k_splits - 1) / a.k_splits;
    const int r_begin = min(part * rows_per, rows_total), r_end = min(r_begin + rows_per, rows_total);
    const int segs = (W + CB_KP - 1) / CB_KP;
    const int nsteps = (r_end - r_begin) * segs;

    // staging roles.  dY: uint4 idx = tid + 256 j (j < 4): pixel r = idx >> 5, and of its 512 bytes (4 chunks of [hi 64 B | lo 64 B])
    // chunk cc = (idx >> 3) & 3, half hl = (idx >> 2) & 1, slot s = idx & 3.  X: halo pixel idx >> 3 (102 of the 128 staged rows), half (idx >> 2) & 1, slot idx & 3.
    // LDS slots: pixel r + 8 j flips bit 1 of the dY swizzle for odd j only, halo pixel + 32 j leaves the X swizzle alone
    int g_lds[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int idx = tid + 256 * j;
        const int r = idx >> 5, cc = (idx >> 3) & 3, hl = (idx >> 2) & 1, s = idx & 3;
        const int ch = cc * 4 + s;
        g_lds[j] = hl * CB_G_BYTES + 256 * r + 16 * (ch ^ rac_tr_swz(r));
    }
    // (rows 102 .. 127 of the X image are padding: written with a re-read of the last halo pixel, never read)
    const int x_lds = 2 * CB_G_BYTES + ((tid >> 2) & 1) * CB_X_BYTES + 64 * (tid >> 3) + 16 * ((tid & 3) ^ (2 * ((tid >> 6) & 1)));
    uint4 rg0, rg1, rg2, rg3, rx0, rx1, rx2, rx3;   // (named, and filled / drained by straight-line code: arrays went to scratch)
#define CB_GLOAD1(j_, rg_, rx_)                                                                              \
    do {                                                                                                     \
        const int idx_ = tid + 256 * (j_), r_ = idx_ >> 5;                                                   \
        const size_t pix_ = (rowbase_ + Wp) + min(w0_ + r_, W - 1) + 1;                                      \
        const uint4 v_ = a.gs[pix_ * (CB_COUT / 32 * 8) + ct * 32 + (idx_ & 31)];                            \
        const unsigned m_ = w0_ + r_ < W ? ~0u : 0u;   /* (a mask, not a branch round the load) */             \
        rg_ = make_uint4(v_.x & m_, v_.y & m_, v_.z & m_, v_.w & m_);                                        \
        const int xr_ = min(idx_ >> 3, CB_XROWS - 1), dy_ = xr_ / CB_XCOLS, cx_ = xr_ - dy_ * CB_XCOLS;      \
        const size_t xp_ = rowbase_ + (size_t)dy_ * Wp + min(w0_ + cx_, W + 1);                              \
        rx_ = a.xs[(xp_ * chunks + chunk) * 8 + (idx_ & 7)];                                                 \
    } while (0)
#define CB_GLOAD(step_)                                                                                      \
    do {                                                                                                     \
        const int row_ = (step_) / segs, w0_ = ((step_) - row_ * segs) * CB_KP;                              \
        const int rr_ = r_begin + row_, n_ = rr_ / H, h_ = rr_ - n_ * H;                                     \
        const size_t rowbase_ = ((size_t)n_ * (H + 2) + h_) * Wp;   /* padded row h: the halo's first */      \
        CB_GLOAD1(0, rg0, rx0); CB_GLOAD1(1, rg1, rx1); CB_GLOAD1(2, rg2, rx2); CB_GLOAD1(3, rg3, rx3);      \
    } while (0)
#define CB_LSTORE(buf_)                                                                                      \
    do {                                                                                                     \
        char *S_ = cb_lds + (buf_) * CB_STAGE_BYTES;                                                         \
        *reinterpret_cast<uint4 *>(S_ + g_lds[0]) = rg0; *reinterpret_cast<uint4 *>(S_ + x_lds) = rx0;              \
        *reinterpret_cast<uint4 *>(S_ + g_lds[1]) = rg1; *reinterpret_cast<uint4 *>(S_ + x_lds + 2048) = rx1;       \
        *reinterpret_cast<uint4 *>(S_ + g_lds[0] + 4096) = rg2; *reinterpret_cast<uint4 *>(S_ + x_lds + 4096) = rx2; \
        *reinterpret_cast<uint4 *>(S_ + g_lds[1] + 4096) = rg3; *reinterpret_cast<uint4 *>(S_ + x_lds + 6144) = rx3; \
    } while (0)

    rac_f4v acc[2][2][9];
#pragma unroll
    for (int mm = 0; mm < 2; ++mm)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int t = 0; t < 9; ++t)
                acc[mm][nt][t] = (rac_f4v){0.f, 0.f, 0.f, 0.f};

    // transposed-read addresses: lane 4 q + p of a 16-lane group supplies row q, elements 4 p .. 4 p + 3 of the block's 16 channels,
    // i.e. 16-byte slot (p >> 1) of the block's two, byte 8 (p & 1) in it.  Block blk of lane group lk holds pixels 8 lk + 4 blk + q.
    const int q = li >> 2, p = li & 3;
    int ga[2][2];       // dY, [mm][blk]: byte offset in the hi image (lo: + CB_G_BYTES)
#pragma unroll
    for (int mm = 0; mm < 2; ++mm)
#pragma unroll
        for (int blk = 0; blk < 2; ++blk) {
            const int r = 8 * lk + 4 * blk + q, ch = 2 * (2 * wave + mm) + (p >> 1);
            ga[mm][blk] = 256 * r + 16 * (ch ^ rac_tr_swz(r)) + 8 * (p & 1);
        }
    const int xrow0 = 8 * lk + q;   // X halo row of block 0 at tap (0, 0); tap (dy, dx) adds dy * CB_XCOLS + dx, block 1 adds 4

    if (nsteps > 0) {     // (uniform over the workgroup: the transposed reads below need every lane active)
        CB_GLOAD(0);
        CB_LSTORE(0);
        __syncthreads();
        for (int step = 0; step < nsteps; ++step) {
            const int nxt = step + 1 < nsteps ? step + 1 : step;
            CB_GLOAD(nxt);     // (past the end the last tile is re-fetched: unconditional code)
            const char *S = cb_lds + (step & 1) * CB_STAGE_BYTES;
            rac_h8 ah[2], al[2];
#pragma unroll
            for (int mm = 0; mm < 2; ++mm) {
                ah[mm] = rac_tr_frag(S, ga[mm][0], ga[mm][1]);
                al[mm] = rac_tr_frag(S + CB_G_BYTES, ga[mm][0], ga[mm][1]);
            }
            const char *SX = S + 2 * CB_G_BYTES;
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int r0 = xrow0 + (t / 3) * CB_XCOLS + (t % 3), r1 = r0 + 4;
                rac_h8 bh[2], bl[2];
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const int s = 2 * nt + (p >> 1);
                    const int o0 = 64 * r0 + 16 * (s ^ (2 * ((r0 >> 3) & 1))) + 8 * (p & 1);
                    const int o1 = 64 * r1 + 16 * (s ^ (2 * ((r1 >> 3) & 1))) + 8 * (p & 1);
                    bh[nt] = rac_tr_frag(SX, o0, o1);
                    bl[nt] = rac_tr_frag(SX + CB_X_BYTES, o0, o1);
                }
#pragma unroll
                for (int mm = 0; mm < 2; ++mm)
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        acc[mm][nt][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mm], bl[nt], acc[mm][nt][t], 0, 0, 0);
                        acc[mm][nt][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[mm], bh[nt], acc[mm][nt][t], 0, 0, 0);
                        acc[mm][nt][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[mm], bh[nt], acc[mm][nt][t], 0, 0, 0);
                    }
            }
            CB_LSTORE((step + 1) & 1);      // the stage read during step - 1: free since the barrier that ended it
            __syncthreads();
        }
    }

    // partial sums, unscaled: accumulator tile (mm, nt, tap) has co = 128 ct + 32 wave + 16 mm + 4 lk + r in the lane's registers and
    // ci = 32 chunk + 16 nt + li on the lane (64-byte runs per 16 lanes)
    const int Cin = chunks * 32;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int mm = 0; mm < 2; ++mm)
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int co = CB_TM * ct + 32 * wave + 16 * mm + 4 * lk + r;
                    a.ws[(((size_t)part * 9 + t) * CB_COUT + co) * Cin + chunk * 32 + 16 * nt + li] = acc[mm][nt][t][r];
                }
}

// dW [256][Cin][3][3] = (sum over the k_splits partial sums in ascending order) / (scale of X * scale of dY)
__global__ __launch_bounds__(256) void conv3x3_wgrad_reduce_kernel(const float *__restrict__ ws, const float *__restrict__ amax_x,
                                                                   const float *__restrict__ amax_g, float *__restrict__ dw, int Cin,
                                                                   int k_splits)
{
    const int per = 9 * CB_COUT * Cin;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= per)
        return;
    float s = 0.f;
    for (int p = 0; p < k_splits; ++p)
        s += ws[(size_t)p * per + e];
    const int t = e / (CB_COUT * Cin), rem = e - t * (CB_COUT * Cin);     // rem = co * Cin + ci
    // (two exact power-of-two factors one after the other: their product could leave the float range)
    dw[(size_t)rem * 9 + t] = s * (1.f / rac_act_scale(*amax_x)) * (1.f / rac_act_scale(*amax_g));
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" int rac_conv_pack_cl_fwd(const float *src, const float *amax, void *xs, int N, int C, int H, int W, int c_total,
                                    int c_offset, void *stream)
{
    RAC_CHECK_ARG(N >= 0 && C > 0 && C % 32 == 0 && c_total % 32 == 0 && c_offset >= 0 && c_offset % 32 == 0 && c_offset + C <= c_total,
                  "rac_conv_pack_cl_fwd: channels C=%d c_total=%d c_offset=%d (multiples of 32)", C, c_total, c_offset);
    RAC_CHECK_ARG(H > 0 && W > 0 && (long)N * H * W * (C / 8) < (1l << 39), "rac_conv_pack_cl_fwd: N=%d H=%d W=%d", N, H, W);
    if (N == 0)
        return 0;
    RAC_CHECK_ARG(src && amax && xs, "rac_conv_pack_cl_fwd: null pointer");
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(xs)) & 15) == 0,
                  "rac_conv_pack_cl_fwd: src / xs must be 16-byte aligned");
    const long total = (long)N * H * W * (C / 8);
    hipLaunchKernelGGL(conv_pack_cl_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, amax,
                       reinterpret_cast<_Float16 *>(xs), total, C, H, W, c_total / 32, c_offset / 32);
    return rac_launch_status("rac_conv_pack_cl_fwd");
}

extern "C" int rac_conv3x3_wgrad(const void *xs, const void *gs, const float *amax_x, const float *amax_g, float *workspace, float *dw,
                                 int N, int H, int W, int Cin, int Cout, int k_splits, void *stream)
{
    RAC_CHECK_ARG(Cout == CB_COUT, "rac_conv3x3_wgrad: built for %d output channels (got %d)", CB_COUT, Cout);
    RAC_CHECK_ARG(Cin > 0 && Cin % 32 == 0 && Cin <= 4096, "rac_conv3x3_wgrad: Cin=%d (a multiple of 32, at most 4096)", Cin);
    RAC_CHECK_ARG(N >= 1 && H > 0 && W > 0 && (long)N * (H + 2) * (W + 2) < (1l << 31), "rac_conv3x3_wgrad: N=%d H=%d W=%d", N, H, W);
    RAC_CHECK_ARG(k_splits >= 1 && k_splits <= N * H && (long)k_splits * 2 * (Cin / 32) < (1l << 31),
                  "rac_conv3x3_wgrad: k_splits=%d (1 .. N*H = %d)", k_splits, N * H);
    RAC_CHECK_ARG(xs && gs && amax_x && amax_g && workspace && dw, "rac_conv3x3_wgrad: null pointer");
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(gs)) & 15) == 0,
                  "rac_conv3x3_wgrad: xs / gs must be 16-byte aligned");
    WgradArgs a;
    a.xs = reinterpret_cast<const uint4 *>(xs);
    a.gs = reinterpret_cast<const uint4 *>(gs);
    a.ws = workspace;
    a.N = N; a.H = H; a.W = W; a.chunks = Cin / 32; a.k_splits = k_splits;
    const int lds = 2 * CB_STAGE_BYTES;
    if (const int rc_attr = rac_set_dynamic_lds_once(RAC_ATTR_CONV3X3_WGRAD, reinterpret_cast<const void *>(conv3x3_wgrad_f16x3_kernel), lds))
        return rc_attr;
    hipLaunchKernelGGL(conv3x3_wgrad_f16x3_kernel, dim3((unsigned)(k_splits * 2 * (Cin / 32))), dim3(256), lds, (hipStream_t)stream, a);
    const int per = 9 * CB_COUT * Cin;
    hipLaunchKernelGGL(conv3x3_wgrad_reduce_kernel, dim3((unsigned)((per + 255) / 256)), dim3(256), 0, (hipStream_t)stream, workspace,
                       amax_x, amax_g, dw, Cin, k_splits);
    return rac_launch_status("rac_conv3x3_wgrad");
}
