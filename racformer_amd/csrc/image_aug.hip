// image_aug.hip -- the detector's image preparation for a training step in one launch, gfx950: GpuPhotoMetricDistortion and GridMask
// (models/utils.py:219-305, :8-45 of the reference) with the img_norm_cfg step and the zero padding of extract_feat between them
// (models/racformer.py:198-224).
//
//   ia_prepare_kernel     raw image [n, 3, H, W] -> normalised, padded, masked image [n, 3, Hp, Wp]; every input value is read once
//                         and every output value written once.  A lane owns four adjacent pixels of one row: three 16-byte loads and
//                         three 16-byte stores where the widths and the pointers allow (template VEC), scalar accesses otherwise and
//                         for the groups that straddle the pad columns.
//
// Per pixel, in float32 with the reference's operations one by one (no contraction, IEEE division): RGB = input channels 2, 1, 0;
// + delta; * alpha0; rgb_to_hsv; s * sat; h + hue, wrapped once by -+360; hsv_to_rgb; * alpha1; output channel k = RGB[map[k]]
// (the random permutation, the flip back to BGR and to_rgb folded into one map); (x - mean[k]) / std[k]; 0 outside the grid mask's
// bands and in the pad.  An image whose table row says "no colour" skips everything between the channel flip and the map.
// No atomics, nothing read back, sized by shapes: capturable and bitwise reproducible.
#include "rac_common.h"

#define IA_COLS 9          // table row: colour flag, delta, alpha0, sat, hue, alpha1, map[3] (as floats 0, 1, 2)

struct IaArgs {
    int H, W, Hp, Wp, groups;      // groups = ceil(Wp / 4)
    int d, l, st_h, st_w;          // grid mask: d == 0 means no mask
    int off_h, off_w, bands_h, bands_w;   // crop offset into the 1.5x canvas, hh / d and ww / d
    float mean[3], stdv[3];
    int norm;                      // 0: mean / std are not applied
};

// torch.remainder(a, 1.0): fmod and the sign fix; a - trunc(a) is exact, the fix is one rounding.
__device__ __forceinline__ float ia_mod1(float a)
{
#pragma clang fp contract(off)
    const float r = a - truncf(a);
    return r < 0.f ? __fadd_rn(r, 1.f) : r;
}

// torch.remainder(a, 6.0); a is in [0, 6] on every finite input of the chain
__device__ __forceinline__ float ia_mod6(float a)
{
#pragma clang fp contract(off)
    if (a >= 0.f && a < 6.f)
        return a;
    const float r = fmodf(a, 6.f);
    return (r != 0.f && r < 0.f) ? __fadd_rn(r, 6.f) : r;
}

__device__ __forceinline__ void ia_colour(float &r, float &g, float &b, const float *__restrict__ t)
{
#pragma clang fp contract(off)
    const float delta = t[1], alpha0 = t[2], sat = t[3], hue = t[4], alpha1 = t[5];
    r = __fmul_rn(__fadd_rn(r, delta), alpha0);
    g = __fmul_rn(__fadd_rn(g, delta), alpha0);
    b = __fmul_rn(__fadd_rn(b, delta), alpha0);
    // rgb_to_hsv (:123-175)
    const float r1 = __fdiv_rn(r, 255.f), g1 = __fdiv_rn(g, 255.f), b1 = __fdiv_rn(b, 255.f);
    const float mx = fmaxf(r1, fmaxf(g1, b1)), mn = fminf(r1, fminf(g1, b1));
    const int arg = (r1 >= g1 && r1 >= b1) ? 0 : (g1 >= b1 ? 1 : 2);       // (the first maximum, as torch.max returns it)
    float dc = __fsub_rn(mx, mn);
    float s = __fdiv_rn(dc, __fadd_rn(mx, 1e-8f));
    dc = dc == 0.f ? 1.f : dc;
    const float rc = __fsub_rn(mx, r1), gc = __fsub_rn(mx, g1), bc = __fsub_rn(mx, b1);
    const float hn = arg == 0 ? __fsub_rn(bc, gc)
                   : arg == 1 ? __fadd_rn(__fsub_rn(rc, bc), __fmul_rn(2.f, dc))
                              : __fadd_rn(__fsub_rn(gc, rc), __fmul_rn(4.f, dc));
    float h = __fmul_rn(ia_mod1(__fdiv_rn(__fdiv_rn(hn, dc), 6.f)), 360.f);
    float v = __fmul_rn(mx, 255.f);
    // saturation, hue, one wrap each way (:277-287)
    s = __fmul_rn(s, sat);
    h = __fadd_rn(h, hue);
    h = h > 360.f ? __fsub_rn(h, 360.f) : h;
    h = h < 0.f ? __fadd_rn(h, 360.f) : h;
    // hsv_to_rgb (:178-216)
    h = __fdiv_rn(h, 360.f);
    v = __fdiv_rn(v, 255.f);
    const float h6 = __fmul_rn(h, 6.f);
    const float hi = ia_mod6(floorf(h6));
    const float f = __fsub_rn(ia_mod6(h6), hi);
    const float p = __fmul_rn(v, __fsub_rn(1.f, s));
    const float q = __fmul_rn(v, __fsub_rn(1.f, __fmul_rn(f, s)));
    const float u = __fmul_rn(v, __fsub_rn(1.f, __fmul_rn(__fsub_rn(1.f, f), s)));
    const int k = (int)hi;                             // 0..5 (anything else, from a non-finite pixel, takes sector 0's row)
    r = k == 1 ? q : (k == 2 || k == 3) ? p : k == 4 ? u : v;              // v q p p t v
    g = (k == 1 || k == 2) ? v : k == 3 ? q : (k == 4 || k == 5) ? p : u;  // t v v q p p
    b = (k == 2) ? u : (k == 3 || k == 4) ? v : k == 5 ? q : p;            // p p t v v q
    r = __fmul_rn(__fmul_rn(r, 255.f), alpha1);
    g = __fmul_rn(__fmul_rn(g, 255.f), alpha1);
    b = __fmul_rn(__fmul_rn(b, 255.f), alpha1);
}

// Position p of the 1.5x canvas against the bands [d i + st, d i + st + l), i = 0 .. bands - 1: u = p - st + d is positive (st < d), so
// one unsigned division gives the band (u / d - 1) and the offset inside its period (u % d); a lane then walks its four pixels by
// incrementing the pair.
struct IaBand {
    unsigned b, m;
};
__device__ __forceinline__ IaBand ia_band_at(int p, int st, int d)
{
    const unsigned u = (unsigned)(p - st + d);
    return IaBand{u / (unsigned)d, u % (unsigned)d};
}
__device__ __forceinline__ bool ia_band_in(const IaBand &k, int l, int bands)
{
    return k.b >= 1u && k.b - 1u < (unsigned)bands && k.m < (unsigned)l;
}
__device__ __forceinline__ void ia_band_next(IaBand &k, int d)
{
    if (++k.m == (unsigned)d) {
        k.m = 0;
        ++k.b;
    }
}

// Workgroup: 64 groups of four pixels (256 columns) x 4 rows; blockIdx.x runs over the n * Hp rows, blockIdx.y over the column chunks.
template <bool VEC>
__global__ __launch_bounds__(256) void ia_prepare_kernel(const float *__restrict__ in, const float *__restrict__ table, float *__restrict__ out,
                                                         int rows, const IaArgs a)
{
#pragma clang fp contract(off)
    const int xg = (int)blockIdx.y * 64 + (int)(threadIdx.x & 63), row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (xg >= a.groups || row >= rows)
        return;
    const int img = row / a.Hp, y = row - img * a.Hp;
    const int x0 = xg * 4, nx = min(4, a.Wp - x0);
    const float *tab = table + img * IA_COLS;
    const size_t plane_in = (size_t)a.H * a.W, plane_out = (size_t)a.Hp * a.Wp;
    const float *src = in + (size_t)img * 3 * plane_in + (size_t)y * a.W + x0;
    float *dst = out + (size_t)img * 3 * plane_out + (size_t)y * a.Wp + x0;

    float o[3][4];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            o[c][j] = 0.f;
    const bool row_in = y < a.H;
    const bool row_band = a.d > 0 && ia_band_in(ia_band_at(y + a.off_h, a.st_h, a.d), a.l, a.bands_h);
    if (row_in && x0 < a.W) {
        const int live = min(nx, a.W - x0);                        // pixels of the group inside the image
        float w[3][4];                                             // working channels R, G, B = input planes 2, 1, 0
        if (VEC) {                                                 // (W % 4 == 0: a group inside the image is whole)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const rac_f4 v = rac_ld4_stream(src + (size_t)(2 - c) * plane_in);
                w[c][0] = v.x, w[c][1] = v.y, w[c][2] = v.z, w[c][3] = v.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    w[c][j] = j < live ? src[(size_t)(2 - c) * plane_in + j] : 0.f;
        }
        const bool colour = tab[0] != 0.f;
        const int m0 = (int)tab[6], m1 = (int)tab[7], m2 = (int)tab[8];
        IaBand col = a.d > 0 ? ia_band_at(x0 + a.off_w, a.st_w, a.d) : IaBand{0u, 0u};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bool keep = a.d == 0 || row_band || ia_band_in(col, a.l, a.bands_w);
            if (a.d > 0)
                ia_band_next(col, a.d);
            if (j >= live || !keep)
                continue;                                          // (masked: stays 0)
            float r = w[0][j], g = w[1][j], b = w[2][j];
            if (colour)
                ia_colour(r, g, b, tab);
            float v0 = m0 == 0 ? r : m0 == 1 ? g : b;
            float v1 = m1 == 0 ? r : m1 == 1 ? g : b;
            float v2 = m2 == 0 ? r : m2 == 1 ? g : b;
            if (a.norm) {
                v0 = __fdiv_rn(__fsub_rn(v0, a.mean[0]), a.stdv[0]);
                v1 = __fdiv_rn(__fsub_rn(v1, a.mean[1]), a.stdv[1]);
                v2 = __fdiv_rn(__fsub_rn(v2, a.mean[2]), a.stdv[2]);
            }
            o[0][j] = v0, o[1][j] = v1, o[2][j] = v2;
        }
    }
    if (VEC) {                                                     // (Wp % 4 == 0: every group is whole)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            rac_st4_stream(dst + (size_t)c * plane_out, rac_f4{o[c][0], o[c][1], o[c][2], o[c][3]});
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nx)
                    dst[(size_t)c * plane_out + j] = o[c][j];
    }
}

extern "C" int rac_image_aug_fwd(const float *img, const float *table, float *out, int n, int H, int W, int Hp, int Wp, const float *mean,
                                 const float *stdv, int grid_d, int grid_l, int grid_st_h, int grid_st_w, void *stream)
{
    const char *what = "rac_image_aug_fwd";
    RAC_CHECK_ARG(n >= 0 && H > 0 && W > 0, "%s: n=%d H=%d W=%d", what, n, H, W);
    RAC_CHECK_ARG(Hp >= H && Wp >= W, "%s: the padded size %d x %d is smaller than the image %d x %d", what, Hp, Wp, H, W);
    RAC_CHECK_ARG(n == 0 || (img && table && out), "%s: null pointer", what);
    RAC_CHECK_ARG((mean == nullptr) == (stdv == nullptr), "%s: mean and std come together (both host pointers to 3 floats, or both NULL)", what);
    RAC_CHECK_ARG(grid_d == 0 || (grid_d >= 2 && grid_l >= 1 && grid_l < grid_d && grid_st_h >= 0 && grid_st_h < grid_d && grid_st_w >= 0 &&
                                  grid_st_w < grid_d),
                  "%s: grid mask d=%d l=%d st_h=%d st_w=%d (d = 0 for none; else d >= 2, 1 <= l < d, 0 <= st < d)", what, grid_d, grid_l,
                  grid_st_h, grid_st_w);
    RAC_CHECK_ARG((int64_t)Hp * Wp < ((int64_t)1 << 30), "%s: %d x %d pixels are too many", what, Hp, Wp);
    if (n == 0)
        return 0;
    IaArgs a;
    a.H = H, a.W = W, a.Hp = Hp, a.Wp = Wp, a.groups = (Wp + 3) / 4;
    a.d = grid_d, a.l = grid_l, a.st_h = grid_st_h, a.st_w = grid_st_w;
    const int hh = (int)(1.5 * Hp), ww = (int)(1.5 * Wp);          // (:20-21: int(1.5 * h))
    a.off_h = (hh - Hp) / 2, a.off_w = (ww - Wp) / 2;
    a.bands_h = grid_d ? hh / grid_d : 0, a.bands_w = grid_d ? ww / grid_d : 0;
    a.norm = mean != nullptr;
    for (int c = 0; c < 3; ++c) {
        a.mean[c] = mean ? mean[c] : 0.f;
        a.stdv[c] = stdv ? stdv[c] : 1.f;
    }
    RAC_CHECK_ARG((int64_t)n * Hp < ((int64_t)1 << 31) && (a.groups + 63) / 64 <= 65535, "%s: %d images of %d x %d are too many", what, n, Hp, Wp);
    const int rows = n * Hp;
    const bool vec = W % 4 == 0 && Wp % 4 == 0 && ((uintptr_t)img % 16 == 0) && ((uintptr_t)out % 16 == 0);
    const dim3 grid((unsigned)((rows + 3) / 4), (unsigned)((a.groups + 63) / 64)), block(256);
    if (vec)
        hipLaunchKernelGGL(ia_prepare_kernel<true>, grid, block, 0, (hipStream_t)stream, img, table, out, rows, a);
    else
        hipLaunchKernelGGL(ia_prepare_kernel<false>, grid, block, 0, (hipStream_t)stream, img, table, out, rows, a);
    return rac_launch_status(what);
}
