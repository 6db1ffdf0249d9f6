// split_f16.h -- what the split-precision matrix-core kernels share beyond rac_common.h's vector types (gfx950): the quarter
// fragment of a transposed LDS read, the hi + lo split of eight scaled values, the transposed LDS fragment read with its row swizzle, and the
// combination of the per-image partial maxima.
#pragma once
#include "rac_common.h"

typedef __fp16 rac_q4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
typedef __attribute__((address_space(3))) rac_q4 *rac_lds_q4;

#define RAC_AMAX_PARTS 64      // partial maxima per image (rac_resnet_absmax_fwd): one per lane of a wave

// v(e) * scale = hi + lo for e = 0 .. 7: the scaled value rounded to f16, and the remainder rounded to f16
template <typename V>
__device__ __forceinline__ void rac_split8(V &&v, float scale, rac_h8 &hi, rac_h8 &lo)
{
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float s = v(e) * scale;
        hi[e] = (_Float16)s;
        lo[e] = (_Float16)(s - (float)hi[e]);
    }
}

// One MFMA fragment (8 consecutive k of the lane's row or column) from an LDS image that keeps k OUTERMOST: two ds_read_b64_tr_b16, each
// over 4 rows x 16 columns per 16-lane group, every lane receiving its column's 4 rows.  Needs every lane active.
__device__ __forceinline__ rac_h8 rac_tr_frag(const char *lds, int off0, int off1)
{
    union {
        struct { rac_q4 a, b; } s;
        rac_h8 v;
    } u;
    u.s.a = __builtin_amdgcn_ds_read_tr16_b64_v4f16((rac_lds_q4)(lds + off0));
    u.s.b = __builtin_amdgcn_ds_read_tr16_b64_v4f16((rac_lds_q4)(lds + off1));
    return u.v;
}

// The 16-byte slot ch of row r of such an image (rows of 256 or 512 bytes) sits at slot ch ^ rac_tr_swz(r), masked to the row's slots:
// conflict-free transposed reads (linear_bwd.hip's header has the argument).
__device__ __forceinline__ int rac_tr_swz(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }

// Maximum over an image's RAC_AMAX_PARTS partial maxima, one per lane, taken on the bit patterns (a NaN wins and turns
// rac_act_scale into 1); every lane of the wave returns it.
__device__ __forceinline__ float rac_wave_amax(const float *__restrict__ parts, int lane)
{
    unsigned mb = rac_absbits(parts[lane]);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
        mb = max(mb, (unsigned)__shfl_xor((int)mb, off));
    return __uint_as_float(mb);
}
