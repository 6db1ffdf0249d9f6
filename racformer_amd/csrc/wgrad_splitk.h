// wgrad_splitk.h -- the split-K weight gradient of a channel-first convolution on the f16 matrix cores (gfx950), the part that the
// necks' lateral stage (fpn_lateral_bwd.hip) and the backbone's Bottleneck convolutions (resnet_bwd.hip) share.  Each of the two
// kernels keeps its own loader, tile shape, number of products and bias sums; the rules below are written here once.
//
// K = the pixels of all images in units of 32 pixels of one image, cut into k_splits contiguous ranges, none empty.  A workgroup of
// 256 threads owns one range and a tile of channels, walks the range twice -- maxima, then products -- and writes its partial sums to
// the workspace [k_splits][taps][Cout][Cin] (+ [k_splits][Cout] for db); wg_reduce_kernel adds the ranges in ascending order.
// Staging: thread t holds pixels 8 (t & 3) .. + 7 of row (t >> 2) + 64 j of the unit's block (the rows of g, then those of x).
// Scale: one power of two per row and K range, the row's largest value in [2^13, 2^14); it factors out of a sum over pixels, and the
// two exact factors are multiplied back one after the other in the epilogue (their product could leave the float range).
// LDS: rows of 64 B hi and, HALF bytes further, 64 B lo; 16-byte slot s of row r at wg_slot(r, s): the 16-lane groups of
// ds_read_b128 then touch 16 distinct slots of a 256-byte line.
// No atomics, nothing read back, every sum in one fixed order.
#pragma once
#include "split_f16.h"

__device__ __forceinline__ int wg_slot(int row, int s) { return s ^ (3 * ((row >> 3) & 1)); }

// The scale of a row whose four staging threads hold the partial maxima m: 2^(13 - e) with e = floor(log2(max)), exponent arithmetic
// only (max = 0 / denormal / inf: clamped exponents).  `unscale` receives 2^(e - 13).
__device__ __forceinline__ float wg_row_scale(float m, float &unscale)
{
    m = fmaxf(m, __shfl_xor(m, 1));
    m = fmaxf(m, __shfl_xor(m, 2));
    int eb = (int)((__float_as_uint(m) >> 23) & 255u);
    eb = eb < 14 ? 14 : (eb > 254 ? 254 : eb);
    unscale = __uint_as_float((unsigned)(eb - 13) << 23);
    return __uint_as_float((unsigned)(267 - eb) << 23);
}

// a row's sum over its four staging threads
__device__ __forceinline__ float wg_row_sum(float t)
{
    t += __shfl_xor(t, 1);
    t += __shfl_xor(t, 2);
    return t;
}

// eight pixels v(0) .. v(7) of `row`, slot s_q: scaled, split and stored to the hi and lo images
template <typename V>
__device__ __forceinline__ void wg_stage(char *lds, int half, int row, int s_q, float scale, V &&v)
{
    rac_h8 hi, lo;
    rac_split8(v, scale, hi, lo);
    char *d = lds + row * 64 + 16 * wg_slot(row, s_q);
    *reinterpret_cast<rac_h8 *>(d) = hi;
    *reinterpret_cast<rac_h8 *>(d + half) = lo;
}

// byte offset of lane (li, lk)'s fragment of the MFMA tile whose first row is row0 (a multiple of 16; the next tile: + 1024)
__device__ __forceinline__ int wg_frag_off(int row0, int li, int lk) { return (row0 + li) * 64 + 16 * wg_slot(li, lk); }

// One staged unit: acc[i][j] += A tile i x B tile j.  PRODUCTS = 3: lo*hi + hi*lo + hi*hi, product-major over i (the necks);
// PRODUCTS = 4: lo*lo first, the four of a tile one after the other (the backbone, whose sums can have a single term).
template <int PRODUCTS, int NI, int NJ>
__device__ __forceinline__ void wg_products(const char *lds, int half, int a_off, int b_off, rac_f4v (&acc)[NI][NJ])
{
    static_assert(PRODUCTS == 3 || PRODUCTS == 4, "three or four products");
    rac_h8 ah[NI], al[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        ah[i] = *reinterpret_cast<const rac_h8 *>(lds + a_off + 1024 * i);
        al[i] = *reinterpret_cast<const rac_h8 *>(lds + half + a_off + 1024 * i);
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const rac_h8 bh = *reinterpret_cast<const rac_h8 *>(lds + b_off + 1024 * j);
        const rac_h8 bl = *reinterpret_cast<const rac_h8 *>(lds + half + b_off + 1024 * j);
        if (PRODUCTS == 3) {
#pragma unroll
            for (int i = 0; i < NI; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < NI; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl, acc[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < NI; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh, acc[i][j], 0, 0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bl, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al[i], bh, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bl, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah[i], bh, acc[i][j], 0, 0, 0);
            }
        }
    }
}

// Epilogue.  Accumulator tile (i, j): rows 4 lk + r = co (tile row 16 (NI wave + i) + 4 lk + r), column li = ci (ci0 + 16 j + li):
// per co the 16 lanes li store 64 contiguous bytes.  unscale[] holds the factors of the tile's co rows, then, from xrow0, of its ci rows;
// wp points at row co 0 of the tile in this range's [Cout][Cin] partial sums.
template <int NI, int NJ>
__device__ __forceinline__ void wg_store(float *__restrict__ wp, const float *unscale, int xrow0, const rac_f4v (&acc)[NI][NJ], int ci0,
                                         int Cin, int wave, int li, int lk)
{
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int ci = ci0 + 16 * j + li;
        if (ci < Cin) {
            const float ux = unscale[xrow0 + 16 * j + li];
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int col = 16 * (NI * wave + i) + 4 * lk + r;
                    wp[(size_t)col * Cin + ci] = acc[i][j][r] * unscale[col] * ux;
                }
        }
    }
}

// dW[co][ci][tap] = the k_splits partial sums added in ascending order; db likewise
static __global__ __launch_bounds__(256) void wg_reduce_kernel(const float *__restrict__ ws, const float *__restrict__ wsb,
                                                               float *__restrict__ dw, float *__restrict__ db, int Cout, int Cin,
                                                               int taps, int k_splits)
{
    const long total = (long)Cout * Cin * taps;
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e < total) {
        size_t at = (size_t)e;      // one tap: the workspace is in dW's order (and the necks' launch does no division)
        if (taps > 1) {
            const int tap = (int)(e % taps);
            const long r = e / taps;
            const int ci = (int)(r % Cin), co = (int)(r / Cin);
            at = ((size_t)tap * Cout + co) * Cin + ci;
        }
        float s = 0.f;
        for (int p = 0; p < k_splits; ++p)
            s += ws[(size_t)p * total + at];
        dw[e] = s;
    } else if (db && e < total + Cout) {
        const int co = (int)(e - total);
        float s = 0.f;
        for (int p = 0; p < k_splits; ++p)
            s += wsb[(size_t)p * Cout + co];
        db[co] = s;
    }
}

// The K split of N images of hw pixels, checked: units of 32 pixels per image, units in all, units per range.  hn / wn name the map's
// sides in the message.
struct WgSplit {
    int upi, units, per;
};
static inline int wg_split(const char *what, const char *hn, const char *wn, int N, int h, int w, int k_splits, const void *g,
                           const void *x, const void *workspace, const void *dw, const void *db, WgSplit &s)
{
    s.upi = (h * w + 31) / 32;
    RAC_CHECK_ARG((long)N * s.upi < (1l << 31), "%s: N=%d %s=%d %s=%d (too many K units)", what, N, hn, h, wn, w);
    s.units = N * s.upi;
    RAC_CHECK_ARG(k_splits >= 1 && k_splits <= s.units, "%s: k_splits=%d (1 .. %d units of 32 pixels)", what, k_splits, s.units);
    s.per = (s.units + k_splits - 1) / k_splits;
    RAC_CHECK_ARG((long)(k_splits - 1) * s.per < s.units, "%s: k_splits=%d leaves an empty range (%d units, %d per range)", what,
                  k_splits, s.units, s.per);
    RAC_CHECK_ARG(g && x && workspace && dw, "%s: null pointer", what);
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(workspace) |
                    reinterpret_cast<uintptr_t>(dw) | reinterpret_cast<uintptr_t>(db)) & 3) == 0,
                  "%s: pointers must be 4-byte aligned", what);
    return 0;
}

// the reduce launch that follows the main kernel: workspace = [k_splits][taps][Cout][Cin], then (db) [k_splits][Cout]
static inline void wg_reduce(const float *workspace, const float *wsb, float *dw, float *db, int Cout, int Cin, int taps, int k_splits,
                             hipStream_t st)
{
    const long outs = (long)Cout * Cin * taps + Cout;
    hipLaunchKernelGGL(wg_reduce_kernel, dim3((unsigned)((outs + 255) / 256)), dim3(256), 0, st, workspace, wsb, dw, db, Cout, Cin, taps,
                       k_splits);
}
