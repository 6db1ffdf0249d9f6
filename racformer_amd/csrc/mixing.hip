// mixing.hip -- AdaptiveMixing core as one kernel on the matrix cores (gfx950).
//
// Replaces, per decoder layer, two batched GEMMs, two LayerNorms over [P,64] / [128,64] and two
// ReLUs of AdaptiveMixing.inner_forward (models/racformer_transformer.py:589-603) -- six launches
// that stream the 88 MB sampled features, the 236 MB generated parameters and two 88/118 MB
// intermediates through HBM several times.  Here each (query, group) item is read once
// (x: 24 KB, M: 16 KB, S: 48 KB) and its [128,64] result written once:
//     Y = relu(LN_{[P,64]}(x @ M))        x [P,64], M [64,64]
//     Z = relu(LN_{[128,64]}(S @ Y))      S [128,P]
// parameter_generator and out_proj stay library GEMMs.
//
// Matrix cores: v_mfma_f32_16x16x4_f32 -- f32 in, f32 accumulate, bit-for-bit an fmaf chain, so the
// result has fp32 GEMM accuracy (no bf16 anywhere).  A workgroup = 4 waves = one item; wave w owns
// output columns 16w..16w+15 of both products (6 + 8 accumulator tiles of 16x16).  Operands are
// staged through LDS with row strides chosen so that every MFMA operand read is bank-conflict
// free (x: 68 floats, M / Y: 80, S: P_pad+4); S is staged in two 64-row halves so that two
// workgroups fit in a CU's 160 KB LDS and one's staging overlaps the other's MFMAs.
#include "rac_common.h"
#include <string.h>

#define MIX_C 64        /* channels per group (in and out) */
#define MIX_OUT 128     /* out_points */
#define MIX_PMAX 96     /* max in_points (f8: 4 points x 8 frames x 3 depths) */
#define MIX_XS 68       /* sX row stride  */
#define MIX_MS 80       /* sM / sY row stride */
#define MIX_SS (MIX_PMAX + 4) /* sS row stride */
#define MIX_REGION_A (MIX_PMAX * MIX_XS + MIX_C * MIX_MS)  /* sX | sM, later sY, later the output tile */
#define MIX_LDS_FLOATS (MIX_REGION_A + 64 * MIX_SS + 16)

struct MixArgs {
    const float *x;       // [items_q, G, P, 64]
    const float *params;  // row q at params + (q % period)*ld_params: per group [64*64 | 128*P]
    float *out;           // [items_q, G, 128, 64] (may be null when out_split is given)
    _Float16 *out_split;  // optional: f16 [items_q, G*256, hi 32 | lo 32] = the line image of out * split_scale (rac_outproj_fwd's A operand)
    int nq, G, P, ld_params;
    int period;           // parameter row period: nq (one row per item row), or a divisor of it (rows shared by batch elements)
    float eps, split_scale;
    float param_scale;    // every generated parameter is multiplied by this on load (the split GEMM's power-of-two alpha)
};

__device__ __forceinline__ float mix_wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        v += __shfl_xor(v, off, 64);
    return v;
}

// block-wide sum of one value per thread (4 waves); red[] is 4 floats of LDS
__device__ __forceinline__ float mix_block_sum(float v, float *red, int wave, int lane)
{
    v = mix_wave_sum(v);
    __syncthreads();
    if (lane == 0)
        red[wave] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// copy the finished [128][64] tile from LDS to the fp32 output and / or the f16 split image
__device__ __forceinline__ void mix_write_out(const MixArgs &a, const float *sO, int q, int g, int tid)
{
    if (a.out) {
        float *go = a.out + ((size_t)q * a.G + g) * MIX_OUT * MIX_C;
        for (int i = tid; i < MIX_OUT * MIX_C / 4; i += 256)
            *reinterpret_cast<rac_f4 *>(go + i * 4) = *reinterpret_cast<const rac_f4 *>(sO + i * 4);
    }
    if (a.out_split) {
        // A operand of out_proj as a 3-product split GEMM on the f16 matrix cores (rac_outproj_fwd): per 32 values of K one
        // 128-byte line [hi 32 | lo 32] of out * split_scale.  K = (g, out point, channel), so the item's 128 out points
        // are 256 consecutive lines: 32 KB contiguous per item, every value stored once.
        _Float16 *go = a.out_split + ((size_t)q * a.G + g) * (size_t)(MIX_OUT * 2 * MIX_C);
        for (int i = tid; i < MIX_OUT * MIX_C / 4; i += 256) {
            const rac_f4 v = *reinterpret_cast<const rac_f4 *>(sO + i * 4);
            rac_h4 hi, lo;
            rac_split_f16(v.x * a.split_scale, hi.x, lo.x);
            rac_split_f16(v.y * a.split_scale, hi.y, lo.y);
            rac_split_f16(v.z * a.split_scale, hi.z, lo.z);
            rac_split_f16(v.w * a.split_scale, hi.w, lo.w);
            const int o = i >> 4, c = (i & 15) * 4;
            _Float16 *dst = go + (o * 2 + (c >> 5)) * 64 + (c & 31);
            *reinterpret_cast<rac_h4 *>(dst) = hi;
            *reinterpret_cast<rac_h4 *>(dst + 32) = lo;
        }
    }
}

// What the f32 forward leaves in registers after its second LayerNorm statistics: wave w's columns 16w..16w+15 of
// A = x @ M (6 row tiles) and of B = S @ Y (8 row tiles), each in the 16x16 accumulator layout (row 16m + 4lk + r, column
// 16w + li in register r of tile m), and the two (mean, 1/std) pairs.  Y is then in LDS (region A, row stride MIX_MS) and
// S half 1 in sS.
struct MixF32State {
    rac_f4v acc1[6], acc2[8];
    float mean1, rstd1, mean2, rstd2;
};

// The f32 forward of item (q, g) up to its second LayerNorm statistics -- shared by mixing_c64_kernel and the backward's
// recompute (mixing_c64_bwd_kernel), so both run the same MFMA k-order and the same block sums.
__device__ __forceinline__ void mix_f32_core(const MixArgs &a, float *smem, int q, int g, MixF32State &st)
{
    rac_f4v (&acc1)[6] = st.acc1;
    rac_f4v (&acc2)[8] = st.acc2;
    float *sX = smem;                          // [P_pad][68]
    float *sM = smem + MIX_PMAX * MIX_XS;      // [64][80]
    float *sY = smem;                          // [P_pad][80]   (aliases sX|sM after step 1)
    float *sS = smem + MIX_REGION_A;           // [64][P_pad+4]
    float *red = sS + 64 * MIX_SS;             // 4 floats (+pad)

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int P = a.P;
    const int MT = (P + 15) >> 4;   // 16-row tiles of x / Y
    const int PP = MIX_PMAX;        // rows / K are always padded to 96 with zeros: branch-free MFMA loops
    (void)MT;
    const float *gx = a.x + ((size_t)q * a.G + g) * P * MIX_C;
    const float *gM = a.params + (size_t)(q % a.period) * a.ld_params + (size_t)g * (MIX_C * MIX_C + MIX_OUT * P);
    const float *gS = gM + MIX_C * MIX_C;

    // ---- stage x (zero rows up to PP), M and S half 0 -------------------------------------------
    // All global loads of the prologue are issued back to back into registers (16 x 16 B per thread)
    // and only then written to LDS: one memory round trip per workgroup instead of one per loop trip.
    const int ncol4 = PP >> 2;                 // float4 columns of a staged S row
    const bool s_vec = (P & 3) == 0;           // S rows are 16-byte aligned
    auto load_S = [&](int half, int k) -> rac_f4 {
        // element k of this thread's share of S rows 64*half .. +63 (columns zero-padded to PP)
        const int i = tid + 256 * k;
        rac_f4 v = {0.f, 0.f, 0.f, 0.f};
        if (i < 64 * ncol4) {
            const int r = i / ncol4, c4 = i - r * ncol4;
            const float *src = gS + (size_t)(64 * half + r) * P + c4 * 4;
            if (c4 * 4 + 3 < P) {
                if (s_vec) {
                    v = rac_ld4(src);
                } else {
                    v.x = src[0]; v.y = src[1]; v.z = src[2]; v.w = src[3];
                }
            } else {
                if (c4 * 4 + 0 < P) v.x = src[0];
                if (c4 * 4 + 1 < P) v.y = src[1];
                if (c4 * 4 + 2 < P) v.z = src[2];
            }
        }
        v.x *= a.param_scale; v.y *= a.param_scale; v.z *= a.param_scale; v.w *= a.param_scale;
        return v;
    };
    auto store_S = [&](int k, rac_f4 v) {
        const int i = tid + 256 * k;
        if (i < 64 * ncol4) {
            const int r = i / ncol4, c4 = i - r * ncol4;
            *reinterpret_cast<rac_f4 *>(sS + r * MIX_SS + c4 * 4) = v;
        }
    };
    {
        rac_f4 vx[6], vm[4], vs[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) {          // x: up to 96 rows x 16 float4
            const int i = tid + 256 * k, r = i >> 4, c4 = i & 15;
            vx[k] = (rac_f4){0.f, 0.f, 0.f, 0.f};
            if (r < P)
                vx[k] = rac_ld4(gx + r * MIX_C + c4 * 4);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {          // M: 64 rows x 16 float4
            const int i = tid + 256 * k, r = i >> 4, c4 = i & 15;
            vm[k] = rac_ld4(gM + r * MIX_C + c4 * 4);
            vm[k].x *= a.param_scale; vm[k].y *= a.param_scale; vm[k].z *= a.param_scale; vm[k].w *= a.param_scale;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k)
            vs[k] = load_S(0, k);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int i = tid + 256 * k, r = i >> 4, c4 = i & 15;
            *reinterpret_cast<rac_f4 *>(sX + r * MIX_XS + c4 * 4) = vx[k];   // rows >= P are zeros
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = tid + 256 * k, r = i >> 4, c4 = i & 15;
            *reinterpret_cast<rac_f4 *>(sM + r * MIX_MS + c4 * 4) = vm[k];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k)
            store_S(k, vs[k]);
    }
    __syncthreads();

    // ---- step 1: Y = x @ M, wave w -> columns 16w.. ---------------------------------------------
#pragma unroll
    for (int m = 0; m < 6; ++m)
        acc1[m] = (rac_f4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int s = 0; s < MIX_C / 4; ++s) {
        const float bv = sM[(4 * s + lk) * MIX_MS + 16 * wave + li];
        float av[6];
#pragma unroll
        for (int m = 0; m < 6; ++m)
            av[m] = sX[(16 * m + li) * MIX_XS + 4 * s + lk];
#pragma unroll
        for (int m = 0; m < 6; ++m)
            acc1[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv, acc1[m], 0, 0, 0);
    }
    // LayerNorm over the P x 64 valid elements (rows >= P are padding: exact zeros, excluded)
    float part = 0.f;
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            part += (16 * m + lk * 4 + r < P) ? acc1[m][r] : 0.f;
    const float n1 = (float)(P * MIX_C);
    const float mean1 = mix_block_sum(part, red, wave, lane) / n1;
    st.mean1 = mean1;
    part = 0.f;
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = acc1[m][r] - mean1;
            part += (16 * m + lk * 4 + r < P) ? d * d : 0.f;
        }
    const float rstd1 = 1.f / sqrtf(mix_block_sum(part, red, wave, lane) / n1 + a.eps);
    st.rstd1 = rstd1;
    // (the two block sums above end with barriers: every wave is past its last sX / sM read)
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * m + lk * 4 + r;
            const float y = rac_relu((acc1[m][r] - mean1) * rstd1);
            sY[row * MIX_MS + 16 * wave + li] = row < P ? y : 0.f;
        }
    __syncthreads();

    // ---- step 2: Z = S @ Y in two 64-row halves --------------------------------------------------
#pragma unroll
    for (int m = 0; m < 8; ++m)
        acc2[m] = (rac_f4v){0.f, 0.f, 0.f, 0.f};
    rac_f4 vs1[6];  // S half 1, fetched while half 0 is being multiplied
#pragma unroll
    for (int k = 0; k < 6; ++k)
        vs1[k] = load_S(1, k);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        if (half == 1) {
            __syncthreads();  // all waves done reading S half 0
#pragma unroll
            for (int k = 0; k < 6; ++k)
                store_S(k, vs1[k]);
            __syncthreads();
        }
#pragma unroll 4
        for (int s = 0; s < MIX_PMAX / 4; ++s) {
            const float bv = sY[(4 * s + lk) * MIX_MS + 16 * wave + li];
            float av[4];
#pragma unroll
            for (int m = 0; m < 4; ++m)
                av[m] = sS[(16 * m + li) * MIX_SS + 4 * s + lk];
#pragma unroll
            for (int m = 0; m < 4; ++m)
                acc2[4 * half + m] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bv, acc2[4 * half + m], 0, 0, 0);
        }
    }
    part = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            part += acc2[m][r];
    const float n2 = (float)(MIX_OUT * MIX_C);
    const float mean2 = mix_block_sum(part, red, wave, lane) / n2;
    st.mean2 = mean2;
    part = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = acc2[m][r] - mean2;
            part += d * d;
        }
    st.rstd2 = 1.f / sqrtf(mix_block_sum(part, red, wave, lane) / n2 + a.eps);
}

__global__ __launch_bounds__(256, 2) void mixing_c64_kernel(const MixArgs a)
{
    extern __shared__ float smem[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int item = blockIdx.x;
    const int q = item / a.G, g = item % a.G;
    MixF32State st;
    mix_f32_core(a, smem, q, g, st);
    // stage the normalised [128][64] tile through LDS (region A is free: Y is dead) for 16-byte stores
    float *sO = smem;  // [128][64], 8192 floats <= MIX_REGION_A
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            sO[(16 * m + lk * 4 + r) * MIX_C + 16 * wave + li] = rac_relu((st.acc2[m][r] - st.mean2) * st.rstd2);
    __syncthreads();
    mix_write_out(a, sO, q, g, tid);
}

// ------------------------------------------------------------------------------------------------
// Backward of the f32 core (rac_mixing_bwd).  One workgroup per (query, group) item recomputes A, Y and B with
// mix_f32_core -- the forward's own arithmetic, so the ReLU masks are the forward's bits -- and then, with B^ = (B-mu2) r2
// and A^ = (A-mu1) r1 (rows >= P excluded from every mean):
//     g2 = dZ [B^ > 0],  dB = r2 (g2 - mean g2 - B^ mean(g2 B^))     dS = dB Y^T [128,P],  dY = S^T dB [P,64]
//     g1 = dY [A^ > 0],  dA = r1 (g1 - mean g1 - A^ mean(g1 A^))     dM = x^T dA [64,64],  dx = dA M^T [P,64]
// LDS plan: the forward's 72 KB (two workgroups per CU), nothing more.  dB stays in the accumulators and goes through LDS a
// 32-row quarter at a time (the 8.5 KB between Y and sS); the quarters run in the order 2, 3, 0, 1 so that the S half the
// recompute left in sS serves the first two, and half 0 is re-read (from L2) for the last two.  For the last two products
// x and M are re-read into region A and dA is written over sS.  dM takes dA straight from the accumulators as its B operand
// (k = 16m + 4lk + r: the accumulator rows of the lane).  Every output element has one writer; no atomics.
#define MIXB_DBS 68                           /* dB quarter row stride */
#define MIXB_DB_OFF (MIX_PMAX * MIX_MS)       /* dB quarter [32][68]: after Y in region A */
#define MIXB_MS 68                            /* re-read M row stride */
#define MIXB_DAS 66                           /* dA row stride (over sS) */

struct MixBwdArgs {
    MixArgs f;                 // x, params, ld_params, nq, G, P, eps as for the forward (param_scale 1, out unused)
    const float *grad_out;     // [nq, G, 128, 64]
    float *grad_x;             // [nq, G, P, 64]
    float *grad_params;        // row q at grad_params + q*ld_grad_params: per group [dM 64*64 | dS 128*P]
    float *z_out;              // optional [nq, G, 128, 64]: the recomputed Z
    int ld_grad_params;
};

__global__ __launch_bounds__(256, 2) void mixing_c64_bwd_kernel(const MixBwdArgs b)
{
    extern __shared__ float smem[];
    const MixArgs &a = b.f;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int P = a.P;
    const int item = blockIdx.x;
    const int q = item / a.G, g = item % a.G;
    float *sY = smem;                                   // [96][80] after the recompute
    float *sDB = smem + MIXB_DB_OFF;                    // [32][68]
    float *sS = smem + MIX_REGION_A;                    // [64][100]
    float *red = sS + 64 * MIX_SS;
    const size_t item_off = (size_t)q * a.G + g;
    const float *gM = a.params + (size_t)(q % a.period) * a.ld_params + (size_t)g * (MIX_C * MIX_C + MIX_OUT * P);
    const float *gS = gM + MIX_C * MIX_C;
    const float *gdz = b.grad_out + item_off * MIX_OUT * MIX_C;
    float *gdM = b.grad_params + (size_t)q * b.ld_grad_params + (size_t)g * (MIX_C * MIX_C + MIX_OUT * P);
    float *gdS = gdM + MIX_C * MIX_C;

    MixF32State st;
    mix_f32_core(a, smem, q, g, st);

    // ---- LN2 + ReLU backward: dB (wave w: columns 16w.., all 128 rows, in the layout of B) ---------------------------
    rac_f4v dB[8];
    float s_g = 0.f, s_gb = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * m + lk * 4 + r, col = 16 * wave + li;
            const float bh = (st.acc2[m][r] - st.mean2) * st.rstd2;
            if (b.z_out)
                b.z_out[item_off * MIX_OUT * MIX_C + row * MIX_C + col] = rac_relu(bh);
            const float g2 = bh > 0.f ? gdz[row * MIX_C + col] : 0.f;
            s_g += g2;
            s_gb += g2 * bh;
            dB[m][r] = g2;
        }
    const float n2 = (float)(MIX_OUT * MIX_C);
    const float mg2 = mix_block_sum(s_g, red, wave, lane) / n2;
    const float mgb2 = mix_block_sum(s_gb, red, wave, lane) / n2;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float bh = (st.acc2[m][r] - st.mean2) * st.rstd2;
            dB[m][r] = st.rstd2 * (dB[m][r] - mg2 - bh * mgb2);
        }

    // ---- dS = dB Y^T and dY = S^T dB, a 32-row quarter of dB at a time ------------------------------------------------
    // dS: wave w -> rows 16(w&1).. of the quarter, out-point columns 48(w>>1).. (3 tiles);  dY: wave w -> columns 16w..
    rac_f4v dY[6];
#pragma unroll
    for (int m = 0; m < 6; ++m)
        dY[m] = (rac_f4v){0.f, 0.f, 0.f, 0.f};
    const int ncol4 = MIX_PMAX >> 2;
    const bool s_vec = (P & 3) == 0;
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int j = (jj + 2) & 3;              // quarters 2, 3 (S half 1, left in sS by the recompute), then 0, 1
        __syncthreads();                         // every wave is past its reads of the previous quarter (and of sS half 1)
        if (jj == 2) {                           // S half 0 into sS (zero-padded columns, as the forward stages it)
            for (int i = tid; i < 64 * ncol4; i += 256) {
                const int r = i / ncol4, c4 = i - r * ncol4;
                const float *src = gS + (size_t)r * P + c4 * 4;
                rac_f4 v = {0.f, 0.f, 0.f, 0.f};
                if (c4 * 4 + 3 < P) {
                    if (s_vec) {
                        v = rac_ld4(src);
                    } else {
                        v.x = src[0]; v.y = src[1]; v.z = src[2]; v.w = src[3];
                    }
                } else {
                    if (c4 * 4 + 0 < P) v.x = src[0];
                    if (c4 * 4 + 1 < P) v.y = src[1];
                    if (c4 * 4 + 2 < P) v.z = src[2];
                }
                *reinterpret_cast<rac_f4 *>(sS + r * MIX_SS + c4 * 4) = v;
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                sDB[(16 * h + lk * 4 + r) * MIXB_DBS + 16 * wave + li] = dB[2 * j + h][r];
        __syncthreads();
        // dS tiles of the quarter
        {
            const int mo = wave & 1, n0 = 3 * (wave >> 1);
            rac_f4v acc[3];
#pragma unroll
            for (int n = 0; n < 3; ++n)
                acc[n] = (rac_f4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
            for (int s = 0; s < MIX_C / 4; ++s) {
                const float av = sDB[(16 * mo + li) * MIXB_DBS + 4 * s + lk];
#pragma unroll
                for (int n = 0; n < 3; ++n)
                    acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, sY[(16 * (n0 + n) + li) * MIX_MS + 4 * s + lk], acc[n], 0, 0, 0);
            }
#pragma unroll
            for (int n = 0; n < 3; ++n) {
                const int p = 16 * (n0 + n) + li;
                if (p < P)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        gdS[(size_t)(32 * j + 16 * mo + lk * 4 + r) * P + p] = acc[n][r];
            }
        }
        // dY += S[32j.., :]^T dB[32j.., :]
        const float *sSq = sS + 32 * (j & 1) * MIX_SS;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const float bv = sDB[(4 * s + lk) * MIXB_DBS + 16 * wave + li];
#pragma unroll
            for (int m = 0; m < 6; ++m)
                dY[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(sSq[(4 * s + lk) * MIX_SS + 16 * m + li], bv, dY[m], 0, 0, 0);
        }
    }

    // ---- LN1 + ReLU backward: dA (wave w: columns 16w.., rows >= P zero) -----------------------------------------------
    // x and M are requested now and land while the statistics are formed
    const float *gx = a.x + item_off * P * MIX_C;
    rac_f4 vx[6], vm[4];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int i = tid + 256 * k, r = i >> 4, c4 = i & 15;
        vx[k] = (rac_f4){0.f, 0.f, 0.f, 0.f};
        if (r < P)
            vx[k] = rac_ld4(gx + r * MIX_C + c4 * 4);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + 256 * k, r = i >> 4, c4 = i & 15;
        vm[k] = rac_ld4(gM + r * MIX_C + c4 * 4);
    }
    float s_g1 = 0.f, s_ga = 0.f;
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * m + lk * 4 + r;
            const float ah = (st.acc1[m][r] - st.mean1) * st.rstd1;
            const float g1 = (row < P && ah > 0.f) ? dY[m][r] : 0.f;
            s_g1 += g1;
            s_ga += g1 * ah;
            dY[m][r] = g1;
        }
    const float n1 = (float)(P * MIX_C);
    const float mg1 = mix_block_sum(s_g1, red, wave, lane) / n1;
    const float mga1 = mix_block_sum(s_ga, red, wave, lane) / n1;
    // (the block sums end with barriers: every wave is past its reads of Y, dB and S)
    float *sX = smem;                          // [96][68]
    float *sMb = smem + MIX_PMAX * MIX_XS;     // [64][68]
    float *sDA = sS;                           // [96][66]
    rac_f4v dA[6];
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * m + lk * 4 + r;
            const float ah = (st.acc1[m][r] - st.mean1) * st.rstd1;
            const float d = row < P ? st.rstd1 * (dY[m][r] - mg1 - ah * mga1) : 0.f;
            dA[m][r] = d;
            sDA[row * MIXB_DAS + 16 * wave + li] = d;
        }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int i = tid + 256 * k, r = i >> 4, c4 = i & 15;
        *reinterpret_cast<rac_f4 *>(sX + r * MIX_XS + c4 * 4) = vx[k];   // rows >= P are zeros
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = tid + 256 * k, r = i >> 4, c4 = i & 15;
        *reinterpret_cast<rac_f4 *>(sMb + r * MIXB_MS + c4 * 4) = vm[k];
    }
    __syncthreads();

    // ---- dM = x^T dA: wave w -> columns 16w.. (its own dA columns, straight from the accumulators) ---------------------
    {
        rac_f4v acc[4];
#pragma unroll
        for (int mc = 0; mc < 4; ++mc)
            acc[mc] = (rac_f4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < 6; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float *xr = sX + (16 * m + 4 * lk + r) * MIX_XS + li;
#pragma unroll
                for (int mc = 0; mc < 4; ++mc)
                    acc[mc] = __builtin_amdgcn_mfma_f32_16x16x4f32(xr[16 * mc], dA[m][r], acc[mc], 0, 0, 0);
            }
#pragma unroll
        for (int mc = 0; mc < 4; ++mc)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                gdM[(16 * mc + lk * 4 + r) * MIX_C + 16 * wave + li] = acc[mc][r];
    }
    // ---- dx = dA M^T: wave w -> columns 16w.. ---------------------------------------------------------------------------
    {
        rac_f4v acc[6];
#pragma unroll
        for (int m = 0; m < 6; ++m)
            acc[m] = (rac_f4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int s = 0; s < MIX_C / 4; ++s) {
            const float bv = sMb[(16 * wave + li) * MIXB_MS + 4 * s + lk];
#pragma unroll
            for (int m = 0; m < 6; ++m)
                acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(sDA[(16 * m + li) * MIXB_DAS + 4 * s + lk], bv, acc[m], 0, 0, 0);
        }
        float *gdx = b.grad_x + item_off * P * MIX_C;
#pragma unroll
        for (int m = 0; m < 6; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * m + lk * 4 + r;
                if (row < P)
                    gdx[row * MIX_C + 16 * wave + li] = acc[m][r];
            }
    }
}

// ------------------------------------------------------------------------------------------------
// Split-precision variant: the same two products on the 16-bit matrix cores (v_mfma_f32_16x16x32_{bf16,f16}) with
// every operand split into 16-bit terms and the leading cross products accumulated in fp32 -- fp32-GEMM accuracy
// at a fraction of the matrix-core time of the f32-input MFMA, which leaves the kernel bound by its 0.4 GB of
// HBM traffic per launch.
//   * x @ M: both operands as three bf16 terms (24 significant bits, fp32 exponent range: the sampled image
//     features are data, nothing bounds them), the six products down to 2^-16 relative kept (truncation 2^-23);
//   * S @ Y: two f16 terms each (22 bits), products hi*hi + hi*lo + lo*hi (truncation 2^-22).  Y is LayerNorm
//     output (|Y| < 79); |S| is bounded by the caller from the generator's weights (AdaptiveMixing.split_packs) -- from above
//     only.  S * param_scale is split as it is, so below |S| = 2^-3 its lo half is an f16 subnormal and S carries an absolute
//     error of up to 2^-25 whatever its size, which the second LayerNorm magnifies as it brings B back to O(1).  Measured
//     (tests/test_mixing_fwd_f64_gpu.py, profiles/mixing_fwd_f64.json; error in units of 2^-24 of the largest output, the
//     float32 restatement's own is 3.3 - 5.9 throughout): 3.2 - 5.2 for std(S) >= 2^-4, 17 - 19 at 2^-6, 56 - 76 at 2^-8,
//     220 - 245 at 2^-10, 870 - 1090 at 2^-12: fp32 grade (within 4 x the restatement's error) down to std(S) = 2^-6, not below;
//     by the tests' criterion with the subnormal floor taken out of its representation term, outside from 2^-8 down at P = 7
//     and at 2^-12 at P = 96.  A per-item power-of-two scale of S (rac_act_scale of the item's max |S|, B multiplied by the
//     exact inverse) removes this and was measured at +1.0 us on 83.5 us per f8 launch against a run-to-run spread of 0.2 us
//     (profiles/mixing_fwd_s_scale_ab.json): left out, the tests assert the kernel to be as accurate as this representation allows;
//   * x and S are converted once while being staged (LDS holds the 16-bit images, conflict-free row strides
//     of 160 / 224 bytes for ds_read_b128 fragment reads);
//   * wave w's slab of M (64 x 16) goes straight from global memory into B fragments (no LDS);
//   * Y never leaves the registers: a 16x16 accumulator tile has its column on the lane and rows 4*lk..4*lk+3 in
//     its 4 registers, so tiles (2t, 2t+1) ARE the B fragment of k-step t of the second product once converted,
//     with k = 32t + 16h + 4lk + i  <->  fragment element 4h + i.  S is staged with that same k permutation
//     (an 8-byte-granular shuffle inside each 32-wide block), so its A fragments stay single 16-byte reads.
typedef __bf16 mix_b8 __attribute__((ext_vector_type(8)));
struct alignas(8) mix_b4 {
    __bf16 x, y, z, w;
};
// v = t1 + t2 + t3 exactly to 24 bits, each term a bf16 (round-to-nearest)
__device__ __forceinline__ void mix_split_bf16(float v, __bf16 &t1, __bf16 &t2, __bf16 &t3)
{
    t1 = (__bf16)v;
    const float r1 = v - (float)t1;
    t2 = (__bf16)r1;
    t3 = (__bf16)(r1 - (float)t2);
}

#define MIXH_XS 80    /* f16 row stride of the x images  (160 B) */
#define MIXH_SS 104   /* f16 row stride of the S images  (208 B) */
#define MIXH_X_BYTES (3 * MIX_PMAX * MIXH_XS * 2)   /* three bf16 terms: 46080 */
#define MIXH_S_BYTES (2 * MIX_OUT * MIXH_SS * 2)    /* hi + lo of all 128 rows: 53248 */
/* the x images (step 1), the S images (step 2) and the output tile (epilogue) take turns in ONE region: 53 KB, so three
   workgroups share a CU's 160 KB */
#define MIXH_REGION_BYTES (MIXH_S_BYTES > MIXH_X_BYTES ? MIXH_S_BYTES : MIXH_X_BYTES)
#define MIXH_LDS_BYTES (MIXH_REGION_BYTES + 64)

// relu(d * 2 * half_r) as rac_relu gives it -- a NaN stays a NaN, every other result is fmaxf's bits -- at fmaxf's cost.  With
// h = d * half_r (half_r = 0.5f / std: the halving is exact), h + |h| is 2h for h > 0, +0 for h <= 0 (-0 included) and NaN for a
// NaN; doubling is exact too, so 2h is the rounded d / std itself (only a result below 2^-125, a subnormal h, may lose its last
// bit).  rac_relu's compare and select on top of the maximum cost this kernel 3 % of its time (profiles/mixing_fwd_s_scale_ab.json).
__device__ __forceinline__ float mix_relu_ln(float d, float half_r)
{
#pragma clang fp contract(off)   // (fma(d, half_r, |h|) would add the product's rounding error where the sum has to be 2h or 0)
    const float h = d * half_r;
    return h + fabsf(h);
}

__device__ __forceinline__ void mix_split4(const rac_f4 v, float scale, rac_h4 &hi, rac_h4 &lo)
{
    rac_split_f16(v.x * scale, hi.x, lo.x);
    rac_split_f16(v.y * scale, hi.y, lo.y);
    rac_split_f16(v.z * scale, hi.z, lo.z);
    rac_split_f16(v.w * scale, hi.w, lo.w);
}

__global__ __launch_bounds__(256, 3) void mixing_c64_f16x3_kernel(const MixArgs a)
{
    extern __shared__ float smem[];
    unsigned char *lds = reinterpret_cast<unsigned char *>(smem);
    __bf16 *sX1 = reinterpret_cast<__bf16 *>(lds);                         // [96][80] x 3 terms
    __bf16 *sX2 = sX1 + MIX_PMAX * MIXH_XS;
    __bf16 *sX3 = sX2 + MIX_PMAX * MIXH_XS;
    _Float16 *sSh = reinterpret_cast<_Float16 *>(lds);                     // [128][104] hi, then lo: over the x images
    _Float16 *sSl = sSh + MIX_OUT * MIXH_SS;
    float *red = reinterpret_cast<float *>(lds + MIXH_REGION_BYTES);

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int P = a.P;
    // the (query, group) items are walked from the LAST one: the generator wrote those rows last, so part of them is still in the
    // Infinity Cache (measured against write order, profiles/r04_mixing_reverse_ab.json: 96.4-97.7 -> 91.2-92.2 us per launch)
    const int item = (int)(gridDim.x - 1 - blockIdx.x);
    const int q = item / a.G, g = item % a.G;
    const float *gx = a.x + ((size_t)q * a.G + g) * P * MIX_C;
    const float *gM = a.params + (size_t)(q % a.period) * a.ld_params + (size_t)g * (MIX_C * MIX_C + MIX_OUT * P);
    const float *gS = gM + MIX_C * MIX_C;
    const float ps = a.param_scale;

    // ---- all global loads of the item are issued up front (22 x 16 B + 16 x 4 B per thread) ------------------
    const bool s_vec = (P & 3) == 0;
    auto load_S = [&](int half, int k) -> rac_f4 {     // float4 number tid+256k of S rows 64*half.. (24 per row, zero-padded)
        const int i = tid + 256 * k;
        const int r = i / 24, c4 = i - r * 24;
        const float *src = gS + (size_t)(64 * half + r) * P + c4 * 4;
        rac_f4 v = {0.f, 0.f, 0.f, 0.f};
        if (c4 * 4 + 3 < P) {
            if (s_vec) {
                v = rac_ld4_stream(src);
            } else {
                v.x = src[0]; v.y = src[1]; v.z = src[2]; v.w = src[3];
            }
        } else {
            if (c4 * 4 + 0 < P) v.x = src[0];
            if (c4 * 4 + 1 < P) v.y = src[1];
            if (c4 * 4 + 2 < P) v.z = src[2];
        }
        return v;
    };
    auto store_S = [&](_Float16 *dh, _Float16 *dl, int k, const rac_f4 v) {
        const int i = tid + 256 * k;
        const int r = i / 24, c4 = i - r * 24;
        // k = 4*c4 = 32t + 16h + 4lk'  ->  column 32t + 8lk' + 4h  (the accumulator-as-operand k order)
        const int t = c4 >> 3, rem = c4 & 7, col = 32 * t + 8 * (rem & 3) + 4 * (rem >> 2);
        rac_h4 hi, lo;
        mix_split4(v, ps, hi, lo);
        *reinterpret_cast<rac_h4 *>(dh + r * MIXH_SS + col) = hi;
        *reinterpret_cast<rac_h4 *>(dl + r * MIXH_SS + col) = lo;
    };
    rac_f4 vx[6], vs0[6], vs1[6];
    float mv[2][8];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int i = tid + 256 * k, r = i >> 4, c4 = i & 15;
        vx[k] = (rac_f4){0.f, 0.f, 0.f, 0.f};
        if (r < P)
            vx[k] = rac_ld4_stream(gx + r * MIX_C + c4 * 4);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j)
            mv[ks][j] = __builtin_nontemporal_load(gM + (32 * ks + 8 * lk + j) * MIX_C + 16 * wave + li);
#pragma unroll
    for (int k = 0; k < 6; ++k)
        vs0[k] = load_S(0, k);
#pragma unroll
    for (int k = 0; k < 6; ++k)
        vs1[k] = load_S(1, k);

#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int i = tid + 256 * k, r = i >> 4, c4 = i & 15;
        mix_b4 t1, t2, t3;                                                    // rows >= P are zeros
        mix_split_bf16(vx[k].x, t1.x, t2.x, t3.x);
        mix_split_bf16(vx[k].y, t1.y, t2.y, t3.y);
        mix_split_bf16(vx[k].z, t1.z, t2.z, t3.z);
        mix_split_bf16(vx[k].w, t1.w, t2.w, t3.w);
        *reinterpret_cast<mix_b4 *>(sX1 + r * MIXH_XS + c4 * 4) = t1;
        *reinterpret_cast<mix_b4 *>(sX2 + r * MIXH_XS + c4 * 4) = t2;
        *reinterpret_cast<mix_b4 *>(sX3 + r * MIXH_XS + c4 * 4) = t3;
    }
    mix_b8 bM1[2], bM2[2], bM3[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            __bf16 t1, t2, t3;
            mix_split_bf16(mv[ks][j] * ps, t1, t2, t3);
            bM1[ks][j] = t1;
            bM2[ks][j] = t2;
            bM3[ks][j] = t3;
        }
    __syncthreads();

    // ---- step 1: Y = x @ M, wave w -> columns 16w.. ------------------------------------------------------------
    rac_f4v acc1[6];
#pragma unroll
    for (int m = 0; m < 6; ++m) {
        acc1[m] = (rac_f4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const int off = (16 * m + li) * MIXH_XS + 32 * ks + 8 * lk;
            const mix_b8 a1 = *reinterpret_cast<const mix_b8 *>(sX1 + off);
            const mix_b8 a2 = *reinterpret_cast<const mix_b8 *>(sX2 + off);
            const mix_b8 a3 = *reinterpret_cast<const mix_b8 *>(sX3 + off);
            // smallest terms first
            acc1[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a3, bM1[ks], acc1[m], 0, 0, 0);
            acc1[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, bM2[ks], acc1[m], 0, 0, 0);
            acc1[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, bM3[ks], acc1[m], 0, 0, 0);
            acc1[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a2, bM1[ks], acc1[m], 0, 0, 0);
            acc1[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, bM2[ks], acc1[m], 0, 0, 0);
            acc1[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a1, bM1[ks], acc1[m], 0, 0, 0);
        }
    }
    float part = 0.f;
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            part += (16 * m + lk * 4 + r < P) ? acc1[m][r] : 0.f;
    const float n1 = (float)(P * MIX_C);
    const float mean1 = mix_block_sum(part, red, wave, lane) / n1;
    part = 0.f;
#pragma unroll
    for (int m = 0; m < 6; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = acc1[m][r] - mean1;
            part += (16 * m + lk * 4 + r < P) ? d * d : 0.f;
        }
    const float rstd1 = 1.f / sqrtf(mix_block_sum(part, red, wave, lane) / n1 + a.eps);
    // (both block sums end with barriers: every wave is past its last read of the x images, so the region can
    //  take the S images now; S stayed in registers through step 1)
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        store_S(sSh, sSl, k, vs0[k]);
        store_S(sSh + 64 * MIXH_SS, sSl + 64 * MIXH_SS, k, vs1[k]);
    }
    // Y = relu(LN(.)) -> B fragments of the second product, in registers
    rac_h8 bYh[3], bYl[3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = 2 * t + h, row = 16 * m + lk * 4 + r;
                const float y = row < P ? mix_relu_ln(acc1[m][r] - mean1, 0.5f * rstd1) : 0.f;
                _Float16 yh, yl;
                rac_split_f16(y, yh, yl);
                bYh[t][4 * h + r] = yh;
                bYl[t][4 * h + r] = yl;
            }
    __syncthreads();   // S visible

    // ---- step 2: Z = S @ Y ---------------------------------------------------------------------------------------
    rac_f4v acc2[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        acc2[m] = (rac_f4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int off = (16 * m + li) * MIXH_SS + 32 * t + 8 * lk;
            const rac_h8 ah = *reinterpret_cast<const rac_h8 *>(sSh + off);
            const rac_h8 al = *reinterpret_cast<const rac_h8 *>(sSl + off);
            acc2[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, bYh[t], acc2[m], 0, 0, 0);
            acc2[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bYl[t], acc2[m], 0, 0, 0);
            acc2[m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, bYh[t], acc2[m], 0, 0, 0);
        }
    }
    part = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            part += acc2[m][r];
    const float n2 = (float)(MIX_OUT * MIX_C);
    const float mean2 = mix_block_sum(part, red, wave, lane) / n2;
    part = 0.f;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float d = acc2[m][r] - mean2;
            part += d * d;
        }
    const float rstd2 = 1.f / sqrtf(mix_block_sum(part, red, wave, lane) / n2 + a.eps);
    // every wave is past its S reads: stage the normalised [128][64] tile (32 KB) over the x / S images
    float *sO = smem;
#pragma unroll
    for (int m = 0; m < 8; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            sO[(16 * m + lk * 4 + r) * MIX_C + 16 * wave + li] = mix_relu_ln(acc2[m][r] - mean2, 0.5f * rstd2);
    __syncthreads();
    mix_write_out(a, sO, q, g, tid);
}

// rac_mixing_fwd with a parameter row period: item row q reads parameter row q % period (period == num_query: one row each).
extern "C" int rac_mixing_period_fwd(const float *x, const float *params, float param_scale, float *out, void *out_split,
                                     float split_scale, int ld_params, int period, int num_query, int groups, int in_points,
                                     int channels, int out_points, float eps, int mfma_mode, void *stream)
{
    RAC_CHECK_ARG(mfma_mode == RAC_MIX_F32 || mfma_mode == RAC_MIX_F16X3, "rac_mixing_fwd: mfma_mode=%d", mfma_mode);
    RAC_CHECK_ARG(channels == MIX_C && out_points == MIX_OUT,
                  "rac_mixing_fwd: built for 64 channels per group and 128 out points (got %d, %d)", channels, out_points);
    RAC_CHECK_ARG(in_points >= 1 && in_points <= MIX_PMAX, "rac_mixing_fwd: in_points=%d out of [1,%d]", in_points, MIX_PMAX);
    RAC_CHECK_ARG(num_query >= 0 && groups >= 1, "rac_mixing_fwd: bad sizes");
    RAC_CHECK_ARG(ld_params >= groups * (MIX_C * MIX_C + MIX_OUT * in_points) && ld_params % 4 == 0 &&
                      (MIX_C * MIX_C + MIX_OUT * in_points) % 4 == 0,
                  "rac_mixing_fwd: parameter row stride %d", ld_params);
    RAC_CHECK_ARG(num_query == 0 || (period >= 1 && period <= num_query && num_query % period == 0),
                  "rac_mixing_period_fwd: parameter row period %d does not divide %d rows", period, num_query);
    static_assert(MIX_REGION_A >= MIX_OUT * MIX_C, "output tile must fit region A");
    static_assert(MIX_REGION_A >= MIX_PMAX * MIX_MS, "Y must fit region A");
    if (num_query == 0)
        return 0;
    RAC_CHECK_ARG(x && params && (out || out_split), "rac_mixing_fwd: null pointer");
    MixArgs a;
    a.x = x; a.params = params; a.out = out;
    a.out_split = reinterpret_cast<_Float16 *>(out_split); a.split_scale = split_scale; a.param_scale = param_scale;
    a.nq = num_query; a.G = groups; a.P = in_points; a.ld_params = ld_params; a.eps = eps;
    a.period = period;
    const size_t lds = (size_t)MIX_LDS_FLOATS * sizeof(float);
    if (const int rc_attr = rac_set_dynamic_lds_once(RAC_ATTR_MIXING_F32, reinterpret_cast<const void *>(mixing_c64_kernel), (int)((int)lds)))
        return rc_attr;
    if (mfma_mode == RAC_MIX_F16X3) {
        static_assert(3 * MIXH_LDS_BYTES <= 160 * 1024, "three workgroups per CU");
        static_assert(MIXH_REGION_BYTES >= MIX_OUT * MIX_C * 4, "output tile must fit the shared region");
        static_assert(MIXH_SS >= MIX_PMAX + 8 && (MIXH_SS * 2) % 16 == 0, "S row stride");
        if (const int rc_attr = rac_set_dynamic_lds_once(RAC_ATTR_MIXING_F16, reinterpret_cast<const void *>(mixing_c64_f16x3_kernel), (int)((int)MIXH_LDS_BYTES)))
            return rc_attr;
        hipLaunchKernelGGL(mixing_c64_f16x3_kernel, dim3(num_query * groups), dim3(256), MIXH_LDS_BYTES, (hipStream_t)stream, a);
        return rac_launch_status("rac_mixing_fwd");
    }
    hipLaunchKernelGGL(mixing_c64_kernel, dim3(num_query * groups), dim3(256), lds, (hipStream_t)stream, a);
    return rac_launch_status("rac_mixing_fwd");
}

extern "C" int rac_mixing_fwd(const float *x, const float *params, float param_scale, float *out, void *out_split,
                              float split_scale, int ld_params, int num_query, int groups, int in_points, int channels, int out_points,
                              float eps, int mfma_mode, void *stream)
{
    // (period = max(num_query, 1): one parameter row per item row, and the size checks keep their own messages)
    return rac_mixing_period_fwd(x, params, param_scale, out, out_split, split_scale, ld_params, num_query > 0 ? num_query : 1,
                                 num_query, groups, in_points, channels, out_points, eps, mfma_mode, stream);
}

extern "C" int rac_mixing_bwd(const float *x, const float *params, int ld_params, const float *grad_out, float *grad_x,
                              float *grad_params, int ld_grad_params, float *z_out, int num_query, int groups, int in_points,
                              int channels, int out_points, float eps, void *stream)
{
    RAC_CHECK_ARG(channels == MIX_C && out_points == MIX_OUT,
                  "rac_mixing_bwd: built for 64 channels per group and 128 out points (got %d, %d)", channels, out_points);
    RAC_CHECK_ARG(in_points >= 1 && in_points <= MIX_PMAX, "rac_mixing_bwd: in_points=%d out of [1,%d]", in_points, MIX_PMAX);
    RAC_CHECK_ARG(num_query >= 0 && groups >= 1, "rac_mixing_bwd: bad sizes");
    const long width = (long)groups * (MIX_C * MIX_C + MIX_OUT * in_points);
    RAC_CHECK_ARG(ld_params >= width && ld_params % 4 == 0, "rac_mixing_bwd: parameter row stride %d", ld_params);
    RAC_CHECK_ARG(ld_grad_params >= width, "rac_mixing_bwd: gradient row stride %d", ld_grad_params);
    RAC_CHECK_ARG((long)num_query * groups <= 0x7fffffffL, "rac_mixing_bwd: %d x %d items", num_query, groups);
    static_assert(MIXB_DB_OFF + 32 * MIXB_DBS <= MIX_REGION_A, "dB quarter must fit between Y and sS");
    static_assert(MIX_PMAX * MIX_XS + MIX_C * MIXB_MS <= MIX_REGION_A, "x and M must fit region A");
    static_assert(MIX_PMAX * MIXB_DAS <= 64 * MIX_SS, "dA must fit over sS");
    if (num_query == 0)
        return 0;
    RAC_CHECK_ARG(x && params && grad_out && grad_x && grad_params, "rac_mixing_bwd: null pointer");
    MixBwdArgs b;
    memset(&b, 0, sizeof(b));
    b.f.x = x; b.f.params = params; b.f.param_scale = 1.f;
    b.f.nq = num_query; b.f.G = groups; b.f.P = in_points; b.f.ld_params = ld_params; b.f.eps = eps;
    b.f.period = num_query;
    b.grad_out = grad_out; b.grad_x = grad_x; b.grad_params = grad_params; b.z_out = z_out; b.ld_grad_params = ld_grad_params;
    const size_t lds = (size_t)MIX_LDS_FLOATS * sizeof(float);
    if (const int rc_attr = rac_set_dynamic_lds_once(RAC_ATTR_MIXING_BWD, reinterpret_cast<const void *>(mixing_c64_bwd_kernel), (int)lds))
        return rc_attr;
    hipLaunchKernelGGL(mixing_c64_bwd_kernel, dim3(num_query * groups), dim3(256), lds, (hipStream_t)stream, b);
    return rac_launch_status("rac_mixing_bwd");
}
