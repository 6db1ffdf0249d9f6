// linear_bwd.hip -- what the two big Linears of AdaptiveMixing (parameter_generator 256 -> 65536, out_proj 32768 -> 256) need under
// autograd beside the forward kernels of gemm_split.hip, in the same arithmetic: every operand is v * 2^e = hi + lo (two f16, 22
// significant bits), the products accumulated in fp32 by v_mfma_f32_16x16x32_f16 (gfx950): the three leading ones lo*hi + hi*lo +
// hi*hi in the forward kernels' launches, all four in the weight gradient (see below).
// No float atomics and a fixed summation order everywhere: two runs give the same bits.
//
//   rac_linear_pack_act      fp32 rows [M][K] (row stride in elements) -> the line image [M][K/32][hi 32 | lo 32] of gemm_split.hip,
//                            scaled by rac_act_scale(*amax) with the amax read ON THE DEVICE (rac_absmax_fwd wrote it): the backward
//                            packs gradients whose range no host has seen, without a read-back
//   rac_linear_pack_wt       W [N][K] fp32 -> the line image of W^T, [K][N/32][hi 32 | lo 32], times a host scale: the W operand of
//                            the data gradients (dX = dY W is the forward kernel on W^T's image)
//   rac_linear_reduce        out[m][n] = bias[n] + alpha / rac_act_scale(*amax) * sum_s partials[s][m][n], s ascending: the slices
//                            of rac_outproj_fwd summed in a fixed order and brought back to true units
//   rac_linear_wgrad         C[a][b] = sum_m A[m][a] Bm[m][b]: the weight gradient of either Linear (and the wide bias gradient)
//
// Weight gradient.  One operand is 256 wide (the "narrow" one: dY of out_proj, the query of the generator) and comes as its line
// image (0.9 MB at 900 rows: L2-resident, every workgroup re-reads it); the other is a multiple of 128 wide (Z, 32768; dP, 65536)
// and is read as fp32 exactly ONCE, split into hi / lo on the way into LDS with its device-side amax -- no 236 MB image is written.
// Both operands keep the reduction index m OUTERMOST in memory while an MFMA fragment wants 8 consecutive m per lane, so the
// fragments are read from LDS with ds_read_b64_tr_b16 (conv3x3_bwd.hip is the precedent): a 16-lane group reads 4 rows x 16 columns
// and every lane receives its column's 4 rows; two such reads make one fragment.  Both operands use the same row <-> k assignment
// (lane group lk, element 4 blk + q <-> row 8 lk + 4 blk + q of the step), which is all the product needs.
//   Workgroup = 256 threads = 4 waves, output tile = all 256 narrow columns x 128 wide columns; a wave owns 64 narrow x 128 wide
//   = 4 x 8 accumulator tiles (128 registers).  A workgroup walks ALL rows in ascending order in K-steps of 32 rows (rows past M are
//   staged as zeros): no K split, so no partial sums and one writer per output element; Wd / 128 workgroups (256 for dW_out, 512
//   for dW_gen at the product shape).
//   Staged per step: narrow [32 rows][256] hi and lo (32 KB), wide [32 rows][128] hi and lo (16 KB); two stages (96 KB), global ->
//   registers -> LDS with the loads of step s+1 in flight under the MFMAs of step s, one barrier per step.
//   LDS images (16-byte slots): slot ch of row r at rowbytes * r + 16 (ch ^ (((r & 3) << 2) | ((r >> 2) & 3))), rowbytes = 512
//   (narrow) or 256 (wide).  Why the transposed reads are conflict-free under the 64-bank rule: a 32-lane half of a read is two
//   16-lane groups (lk, lk + 1), each 4 rows x 32 bytes, rows r .. r+3 and r+8 .. r+11 (r a multiple of 4), and the 64 banks are one
//   256-byte window, which every row starts anew (rows are 1 or 2 whole windows).  The XOR puts (r & 3) into bits 2-3 of the slot --
//   four distinct 64-byte quarters of the window for a group's four rows -- and ((r >> 2) & 3), whose bit 1 is what r -> r+8 flips,
//   into bits 0-1: the two groups sit in different 32-byte halves of a quarter (a tile's two slots differ in bit 0 only).  The
//   16 (row, slot) pairs of a half take 16 distinct slots of the window.  All addresses are multiples of 8.
//   Output orientation (template flag): the operand given to the MFMA as A supplies the accumulator's ROWS, four consecutive ones per
//   lane = one 16-byte store.  WIDE_MAJOR = false: C stored [256][Wd] (dW_out; the wide operand is A), true: [Wd][256] (dW_gen; the
//   narrow operand is A).  The fragments of both operands are loaded alike, so the flag only swaps the MFMA's arguments.
//   FOUR products, lo*lo + lo*hi + hi*lo + hi*hi, where the forward kernels take three: a weight gradient over few rows is a sum of
//   few terms -- at M = 1 a single product --, and there the dropped lo*lo term (up to 2^-22 of the product) on top of the two
//   operands' own 2^-22 reaches 12 x 2^-24 of |a||b| in the worst case: measured 8.7 x 2^-24 on 10 of 1.2 M elements of a one-row
//   gradient, outside the 8 x 2^-24 the float64 tests hold every product to.  With the fourth product a single term stays under
//   5 x 2^-24 (4 M simulated pairs).  The data gradients keep the forward kernels' three: their sums have at least 128 terms.
//   Column sums of the wide operand (db_gen = sum_m dP) come from the same pass: the staging threads add the fp32 values they
//   convert (thread t: rows t / 16 and t / 16 + 16 of every step, ascending), and sixteen such row classes are added in ascending
//   order at the end -- a fixed order, one writer per column.
#include "split_f16.h"

#define LB_NARROW 256
#define LB_TW 128                                  /* wide columns per workgroup */
#define LB_KR 32                                   /* rows per K-step */
#define LB_N_BYTES (LB_KR * LB_NARROW * 2)         /* 16384: one of hi / lo of the narrow tile */
#define LB_W_BYTES (LB_KR * LB_TW * 2)             /* 8192: one of hi / lo of the wide tile */
#define LB_STAGE_BYTES (2 * LB_N_BYTES + 2 * LB_W_BYTES)   /* 49152 */

// ------------------------------------------------------------------------------------------------ packs
// One thread = 8 consecutive values of a row: 32 bytes in, 16 bytes of hi and 16 bytes of lo out.
__global__ __launch_bounds__(256) void linear_pack_act_kernel(const float *__restrict__ src, long ld_src, const float *__restrict__ amax,
                                                              _Float16 *__restrict__ img, long total, int K)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total)
        return;
    const int k8n = K >> 3;
    const long row = i / k8n;
    const int k8 = (int)(i - row * k8n);
    const float scale = rac_act_scale(*amax);
    const float *p = src + row * ld_src + k8 * 8;
    const rac_f4 v0 = rac_ld4(p), v1 = rac_ld4(p + 4);
    const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
    rac_h8 hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float s = v[j] * scale;
        hi[j] = (_Float16)s;
        lo[j] = (_Float16)(s - (float)hi[j]);
    }
    _Float16 *o = img + (row * (K >> 5) + (k8 >> 2)) * 64 + (k8 & 3) * 8;
    *reinterpret_cast<rac_h8 *>(o) = hi;
    *reinterpret_cast<rac_h8 *>(o + 32) = lo;
}

// Workgroup = one 32 x 32 tile of W through LDS: read along K (W's rows), written along N (the image's lines).
__global__ __launch_bounds__(256) void linear_pack_wt_kernel(const float *__restrict__ w, _Float16 *__restrict__ img, int N, int K, float scale)
{
    __shared__ float tile[32][33];
    const int n0 = blockIdx.x * 32, k0 = blockIdx.y * 32, t = threadIdx.x;
    {
        const int n = t >> 3, k4 = (t & 7) * 4;
        const rac_f4 v = rac_ld4(w + (size_t)(n0 + n) * K + k0 + k4);
        tile[n][k4] = v.x; tile[n][k4 + 1] = v.y; tile[n][k4 + 2] = v.z; tile[n][k4 + 3] = v.w;
    }
    __syncthreads();
    const int k = t >> 3, n4 = (t & 7) * 4;
    rac_h4 hi, lo;
    rac_split_f16(tile[n4][k] * scale, hi.x, lo.x);
    rac_split_f16(tile[n4 + 1][k] * scale, hi.y, lo.y);
    rac_split_f16(tile[n4 + 2][k] * scale, hi.z, lo.z);
    rac_split_f16(tile[n4 + 3][k] * scale, hi.w, lo.w);
    _Float16 *dst = img + ((size_t)(k0 + k) * (N >> 5) + blockIdx.x) * 64 + n4;
    *reinterpret_cast<rac_h4 *>(dst) = hi;
    *reinterpret_cast<rac_h4 *>(dst + 32) = lo;
}

// out[m][n] = bias[n] + alpha / rac_act_scale(*amax) * (partials[0][m][n] + partials[1][m][n] + ...), one thread per 4 columns
__global__ __launch_bounds__(256) void linear_reduce_kernel(const float *__restrict__ part, const float *__restrict__ bias,
                                                            const float *__restrict__ amax, float alpha, float *__restrict__ out,
                                                            long ld_out, int slices, int M, int N)
{
    const int n4n = N >> 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)M * n4n)
        return;
    const long m = i / n4n;
    const int n = (int)(i - m * n4n) * 4;
    const size_t per = (size_t)M * N;
    const float *p = part + (size_t)m * N + n;
    rac_f4 s = rac_ld4(p);
    for (int k = 1; k < slices; ++k) {
        const rac_f4 v = rac_ld4(p + k * per);
        s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
    // (two exact power-of-two factors one after the other: their product could leave the float range)
    const float inv = 1.f / rac_act_scale(*amax);
    rac_f4 b = {0.f, 0.f, 0.f, 0.f};
    if (bias)
        b = rac_ld4(bias + n);
    rac_f4 o;
    o.x = s.x * alpha * inv + b.x;
    o.y = s.y * alpha * inv + b.y;
    o.z = s.z * alpha * inv + b.z;
    o.w = s.w * alpha * inv + b.w;
    *reinterpret_cast<rac_f4 *>(out + m * ld_out + n) = o;
}

// ------------------------------------------------------------------------------------------------ weight gradient
struct LinWgradArgs {
    const uint4 *nimg;      // narrow operand: line image [M][8 lines][hi 32 | lo 32] f16 (64 uint4 per row)
    const float *wide;      // wide operand: fp32 [M][ld_wide]
    const float *amax_n;    // device max |value| the narrow image was packed with
    const float *amax_w;    // device max |value| of the wide operand
    float *out;             // [256][Wd] or, WIDE_MAJOR, [Wd][256]
    float *colsum;          // [Wd] column sums of the wide operand, or null
    long ld_wide;
    int M, Wd;
};

template <bool WIDE_MAJOR>
__global__ __launch_bounds__(256, 1) void linear_wgrad_split_kernel(const LinWgradArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lb_lds[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lk = lane >> 4;
    const int M = a.M, b0 = blockIdx.x * LB_TW;
    const int nsteps = (M + LB_KR - 1) / LB_KR;
    const float scale_w = rac_act_scale(*a.amax_w);

    // staging roles.  Narrow: uint4 idx = tid + 256 j (j < 8): row r = (tid >> 6) + 4 j of the step, and of its 1 KB (8 lines of
    // [hi 64 B | lo 64 B]) line l = (tid >> 3) & 7, half hl = (tid >> 2) & 1, slot s = tid & 3, i.e. columns 32 l + 8 s .. + 7: LDS slot
    // ch = 4 l + s.  Wide: item = tid + 256 j (j < 2): row r = (tid >> 4) + 16 j, columns 8 (tid & 15) .. + 7 (two float4): LDS slot tid & 15.
    const int n_u = tid & 63, n_rb = tid >> 6, n_ch = 4 * ((tid >> 3) & 7) + (tid & 3), n_hl = (tid >> 2) & 1;
    const int w_rb = tid >> 4, w_ch = tid & 15;
    uint4 rn[8];
    rac_f4v rw[4];
    float cs[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
        cs[e] = 0.f;

    auto gload = [&](int step) {
        const int m0 = step * LB_KR;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int m = m0 + n_rb + 4 * j;
            const uint4 v = a.nimg[(size_t)min(m, M - 1) * 64 + n_u];      // rows past M are never read: the last row again, masked
            const unsigned k = m < M ? ~0u : 0u;
            rn[j] = make_uint4(v.x & k, v.y & k, v.z & k, v.w & k);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = m0 + w_rb + 16 * j;
            const float *p = a.wide + (size_t)min(m, M - 1) * a.ld_wide + b0 + 8 * w_ch;
            const rac_f4v v0 = *reinterpret_cast<const rac_f4v *>(p), v1 = *reinterpret_cast<const rac_f4v *>(p + 4);
            const rac_f4v z = {0.f, 0.f, 0.f, 0.f};
            rw[2 * j] = m < M ? v0 : z;          // (a select, not a product: the masked row may hold anything)
            rw[2 * j + 1] = m < M ? v1 : z;
        }
    };
    // `real`: the registers hold a step of the walk (not the re-fetched last one): its values enter the column sums
    auto lstore = [&](int buf, bool real) {
        char *S = lb_lds + buf * LB_STAGE_BYTES;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int r = n_rb + 4 * j;
            *reinterpret_cast<uint4 *>(S + n_hl * LB_N_BYTES + 512 * r + 16 * (n_ch ^ rac_tr_swz(r))) = rn[j];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int r = w_rb + 16 * j;
            rac_h8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = e < 4 ? rw[2 * j][e] : rw[2 * j + 1][e - 4];
                if (real)
                    cs[e] += v;
                const float s = v * scale_w;
                hi[e] = (_Float16)s;
                lo[e] = (_Float16)(s - (float)hi[e]);
            }
            char *d = S + 2 * LB_N_BYTES + 256 * r + 16 * (w_ch ^ rac_tr_swz(r));
            *reinterpret_cast<rac_h8 *>(d) = hi;
            *reinterpret_cast<rac_h8 *>(d + LB_W_BYTES) = lo;
        }
    };

    rac_f4v acc[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            acc[i][j] = (rac_f4v){0.f, 0.f, 0.f, 0.f};

    // transposed-read addresses: lane 4 q + p of a 16-lane group supplies row q, elements 4 p .. 4 p + 3 of the tile's 16 columns, i.e.
    // 16-byte slot (p >> 1) of the tile's two, byte 8 (p & 1) in it.  Block blk of lane group lk holds rows 8 lk + 4 blk + q.
    const int q = li >> 2, p = li & 3;
    int na[4][2], wa[8][2];
#pragma unroll
    for (int blk = 0; blk < 2; ++blk) {
        const int r = 8 * lk + 4 * blk + q, sw = rac_tr_swz(r);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            na[i][blk] = 512 * r + 16 * ((8 * wave + 2 * i + (p >> 1)) ^ sw) + 8 * (p & 1);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            wa[j][blk] = 2 * LB_N_BYTES + 256 * r + 16 * ((2 * j + (p >> 1)) ^ sw) + 8 * (p & 1);
    }

    // (M >= 1: at least one step; uniform over the workgroup -- the transposed reads need every lane active)
    gload(0);
    lstore(0, true);
    __syncthreads();
    for (int step = 0; step < nsteps; ++step) {
        const bool more = step + 1 < nsteps;
        gload(more ? step + 1 : step);      // (past the end the last tile is re-fetched: unconditional code)
        const char *S = lb_lds + (step & 1) * LB_STAGE_BYTES;
        rac_h8 nh[4], nl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            nh[i] = rac_tr_frag(S, na[i][0], na[i][1]);
            nl[i] = rac_tr_frag(S + LB_N_BYTES, na[i][0], na[i][1]);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const rac_h8 wh = rac_tr_frag(S, wa[j][0], wa[j][1]);
            const rac_h8 wl = rac_tr_frag(S + LB_W_BYTES, wa[j][0], wa[j][1]);
            // smallest terms first (all four products: see the header); product-major, so that four independent accumulators lie between two MFMAs into the same one
            if (WIDE_MAJOR) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(nl[i], wl, acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(nl[i], wh, acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(nh[i], wl, acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(nh[i], wh, acc[i][j], 0, 0, 0);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, nl[i], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl, nh[i], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, nl[i], acc[i][j], 0, 0, 0);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh, nh[i], acc[i][j], 0, 0, 0);
            }
        }
        lstore((step + 1) & 1, more);       // the stage read during step - 1: free since the barrier that ended it
        __syncthreads();
    }

    // true units: two exact power-of-two factors one after the other (their product could leave the float range).
    // Accumulator tile (i, j): rows 4 lk + r come from the MFMA's A operand, column li from its B operand.
    const float inv_n = 1.f / rac_act_scale(*a.amax_n), inv_w = 1.f / scale_w;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const rac_f4v v = acc[i][j] * inv_n * inv_w;
            if (WIDE_MAJOR) {
                const int na_ = 64 * wave + 16 * i + 4 * lk, b = b0 + 16 * j + li;
                *reinterpret_cast<rac_f4v *>(a.out + (size_t)b * LB_NARROW + na_) = v;
            } else {
                const int na_ = 64 * wave + 16 * i + li, b = b0 + 16 * j + 4 * lk;
                *reinterpret_cast<rac_f4v *>(a.out + (size_t)na_ * a.Wd + b) = v;
            }
        }

    if (a.colsum) {       // (uniform; the loop's last barrier has freed the stages)
        float *red = reinterpret_cast<float *>(lb_lds);     // [16 row classes][128 columns]
#pragma unroll
        for (int e = 0; e < 8; ++e)
            red[w_rb * LB_TW + 8 * w_ch + e] = cs[e];
        __syncthreads();
        if (tid < LB_TW) {
            float s = red[tid];
            for (int g = 1; g < 16; ++g)
                s += red[g * LB_TW + tid];
            a.colsum[b0 + tid] = s;
        }
    }
}

// ------------------------------------------------------------------------------------------------ C-ABI
extern "C" int rac_linear_pack_act(const float *src, int64_t ld_src, const float *amax, void *image, int M, int K, void *stream)
{
    RAC_CHECK_ARG(M >= 1 && K >= 32 && K % 32 == 0 && ld_src >= K && ld_src % 4 == 0 && (long)M * (K / 8) < (1l << 39),
                  "rac_linear_pack_act: M=%d K=%d ld_src=%lld (K a multiple of 32, ld_src >= K and a multiple of 4)", M, K, (long long)ld_src);
    RAC_CHECK_ARG(src && amax && image, "rac_linear_pack_act: null pointer");
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(image)) & 15) == 0,
                  "rac_linear_pack_act: src / image must be 16-byte aligned");
    const long total = (long)M * (K / 8);
    hipLaunchKernelGGL(linear_pack_act_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, src, (long)ld_src,
                       amax, reinterpret_cast<_Float16 *>(image), total, K);
    return rac_launch_status("rac_linear_pack_act");
}

extern "C" int rac_linear_pack_wt(const float *weight, void *image, int N, int K, float scale, void *stream)
{
    RAC_CHECK_ARG(N >= 32 && N % 32 == 0 && K >= 32 && K % 32 == 0 && K / 32 <= 65535,
                  "rac_linear_pack_wt: N=%d K=%d (multiples of 32, K at most 32 * 65535)", N, K);
    RAC_CHECK_ARG(weight && image, "rac_linear_pack_wt: null pointer");
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(image)) & 15) == 0,
                  "rac_linear_pack_wt: weight / image must be 16-byte aligned");
    hipLaunchKernelGGL(linear_pack_wt_kernel, dim3(N / 32, K / 32), dim3(256), 0, (hipStream_t)stream, weight,
                       reinterpret_cast<_Float16 *>(image), N, K, scale);
    return rac_launch_status("rac_linear_pack_wt");
}

extern "C" int rac_linear_reduce(const float *partials, const float *bias, const float *amax, float alpha, float *out, int64_t ld_out,
                                 int slices, int M, int N, void *stream)
{
    RAC_CHECK_ARG(slices >= 1 && M >= 1 && N >= 4 && N % 4 == 0 && ld_out >= N && ld_out % 4 == 0,
                  "rac_linear_reduce: slices=%d M=%d N=%d ld_out=%lld (N and ld_out multiples of 4, ld_out >= N)", slices, M, N, (long long)ld_out);
    RAC_CHECK_ARG(partials && amax && out, "rac_linear_reduce: null pointer");
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(partials) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(bias)) & 15) == 0,
                  "rac_linear_reduce: partials / bias / out must be 16-byte aligned");
    const long total = (long)M * (N / 4);
    hipLaunchKernelGGL(linear_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, partials, bias, amax,
                       alpha, out, (long)ld_out, slices, M, N);
    return rac_launch_status("rac_linear_reduce");
}

extern "C" int rac_linear_wgrad(const void *narrow_image, const float *amax_narrow, const float *wide, int64_t ld_wide,
                                const float *amax_wide, float *out, float *colsum, int M, int narrow, int Wd, int wide_major, void *stream)
{
    RAC_CHECK_ARG(narrow == LB_NARROW, "rac_linear_wgrad: built for a narrow side of %d (got %d)", LB_NARROW, narrow);
    RAC_CHECK_ARG(Wd >= LB_TW && Wd % LB_TW == 0, "rac_linear_wgrad: wide side %d must be a multiple of %d", Wd, LB_TW);
    RAC_CHECK_ARG(M >= 1 && ld_wide >= Wd && ld_wide % 4 == 0, "rac_linear_wgrad: M=%d ld_wide=%lld (at least the wide side %d, a multiple of 4)", M,
                  (long long)ld_wide, Wd);
    RAC_CHECK_ARG(narrow_image && amax_narrow && wide && amax_wide && out, "rac_linear_wgrad: null pointer");
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(narrow_image) | reinterpret_cast<uintptr_t>(wide) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                  "rac_linear_wgrad: narrow_image / wide / out must be 16-byte aligned");
    LinWgradArgs a;
    a.nimg = reinterpret_cast<const uint4 *>(narrow_image);
    a.wide = wide; a.amax_n = amax_narrow; a.amax_w = amax_wide; a.out = out; a.colsum = colsum;
    a.ld_wide = ld_wide; a.M = M; a.Wd = Wd;
    const int lds = 2 * LB_STAGE_BYTES;
    if (wide_major) {
        if (const int rc = rac_set_dynamic_lds_once(RAC_ATTR_LINEAR_WGRAD_W, reinterpret_cast<const void *>(linear_wgrad_split_kernel<true>), lds))
            return rc;
        hipLaunchKernelGGL(linear_wgrad_split_kernel<true>, dim3(Wd / LB_TW), dim3(256), lds, (hipStream_t)stream, a);
    } else {
        if (const int rc = rac_set_dynamic_lds_once(RAC_ATTR_LINEAR_WGRAD_N, reinterpret_cast<const void *>(linear_wgrad_split_kernel<false>), lds))
            return rc;
        hipLaunchKernelGGL(linear_wgrad_split_kernel<false>, dim3(Wd / LB_TW), dim3(256), lds, (hipStream_t)stream, a);
    }
    return rac_launch_status("rac_linear_wgrad");
}
