// image_geom.hip -- RandomTransformImage of the reference's data pipeline (loaders/pipelines/transforms.py:219-342) in one launch,
// gfx950: the raw uint8 camera frames [n, Hr, Wr, 3] to the cropped, flipped, bicubically resized images the detector takes, as Pillow's
// 8-bit resampler computes them (horizontal pass, vertical pass, each in 22-bit fixed point from 2^21, shifted and clipped to uint8).
//
//   ig_transform_kernel   a workgroup owns a tile of 64 output columns x 16 output rows x 3 channels of one image.  The host's tables
//                         (racformer_amd/image_geom.py: geometry_tables) give, per OUTPUT column and row, the first raw position, the tap
//                         count and the int32 weights -- crop offset and flip are folded in, a position outside the resized image has no
//                         taps -- and per tile column / tile row the span of raw columns / rows its positions read.
//                         1. the raw bytes of the tile's column span are staged into LDS, 16 raw rows at a time, as aligned dwords
//                            (assembled from bytes only where a dword would leave the tensor);
//                         2. the horizontal pass runs from the stage into an LDS image [raw row][channel][column] of uint8, after
//                            Pillow's rounding and clip;
//                         3. the vertical pass runs from that image and stores.
//                         A position without taps sums to 2^21 >> 22 = 0 and reads nothing, so the zero fill outside the resized
//                         image needs no branch.  A skipped pass is one tap of weight 2^22, which returns the byte unchanged.
//
// Integer arithmetic only (an int32 accumulator cannot overflow: the host asserts 255 sum|k| + 2^21 < 2^31 per row); 64-bit offsets;
// the raw image is only read, every output element is written exactly once; no atomics, nothing read back, sized by shapes:
// capturable and bitwise reproducible.  Spans beyond the LDS budget below are refused by the entry point before any launch.
#include "rac_common.h"

#define IG_TILE_W 64
#define IG_TILE_H 16
#define IG_CHUNK 16        // raw rows staged at a time
#define IG_SPAN_DW 160     // dwords of one staged row: 3 * span + 3 (misalignment) bytes have to fit
#define IG_SPAN_PX ((4 * IG_SPAN_DW - 3) / 3)
#define IG_ROWS 64         // raw rows one tile row may read
#define IG_TAPS 16         // taps per output position

struct IgArgs {
    int group, Hr, Wr, fH, fW, ks, ntx, nty, kind;
    long long raw_bytes;
};

__device__ __forceinline__ int ig_clip8(int s)
{
    return min(max(s >> 22, 0), 255);
}

__global__ __launch_bounds__(256) void ig_transform_kernel(const uint8_t *__restrict__ raw, const int32_t *__restrict__ tables, void *__restrict__ out,
                                                           const IgArgs a)
{
    __shared__ uint32_t stage[IG_CHUNK][IG_SPAN_DW];
    __shared__ uint8_t himg[IG_ROWS][3][IG_TILE_W];
    __shared__ int32_t hkl[IG_TAPS][IG_TILE_W];

    const int tid = (int)threadIdx.x, c = tid & 63, q = tid >> 6;
    const int bx = (int)blockIdx.x, by = (int)blockIdx.y, img = (int)blockIdx.z;
    const int stride = 2 * a.fW + 2 * a.fH + 2 * a.ntx + 2 * a.nty + (a.fW + a.fH) * a.ks;
    const int32_t *hb = tables + (int64_t)(img / a.group) * stride, *vb = hb + 2 * a.fW, *tx = vb + 2 * a.fH, *ty = tx + 2 * a.ntx;
    const int32_t *hk = ty + 2 * a.nty, *vk = hk + (int64_t)a.fW * a.ks;
    const int xlo = tx[2 * bx], span = tx[2 * bx + 1] - xlo, r0 = ty[2 * by], nrows = ty[2 * by + 1] - r0;
    const int ox = bx * IG_TILE_W + c;
    const bool col_in = ox < a.fW;
    const int xmin = col_in ? hb[2 * ox] : 0, xcnt = col_in ? hb[2 * ox + 1] : 0;
    for (int t = q; t < xcnt; t += 4)
        hkl[t][c] = hk[(int64_t)ox * a.ks + t];

    // the staged segment of raw row r starts at byte 3 * xlo of the row, moved down to the dword that holds it
    const uintptr_t base = (uintptr_t)raw;
    const int64_t img_row0 = (int64_t)img * a.Hr + r0;
    const int ndw_max = (3 * span + 6) / 4;                        // dwords that cover 3 * span bytes at any misalignment
    for (int ch0 = 0; ch0 < nrows; ch0 += IG_CHUNK) {
        const int rows_here = min(IG_CHUNK, nrows - ch0);
        __syncthreads();                                           // (the previous chunk's stage has been read; hkl is written)
        if (span > 0) {
            for (int i = tid; i < rows_here * ndw_max; i += 256) {
                const int r = i / ndw_max, d = i - r * ndw_max;
                const int64_t first = ((img_row0 + ch0 + r) * a.Wr + xlo) * 3;          // byte offset into raw
                const int lead = (int)((base + (uintptr_t)first) & 3u);
                if (4 * d >= lead + 3 * span)
                    continue;
                const int64_t at = first - lead + 4 * (int64_t)d;                       // this dword's byte offset (may be < 0)
                uint32_t v;
                if (at >= 0 && at + 4 <= a.raw_bytes) {
                    v = *reinterpret_cast<const uint32_t *>(raw + at);
                } else {                                           // (the tensor's first or last bytes: byte by byte)
                    v = 0;
                    for (int b = 0; b < 4; ++b)
                        if (at + b >= 0 && at + b < a.raw_bytes)
                            v |= (uint32_t)raw[at + b] << (8 * b);
                }
                stage[r][d] = v;
            }
        }
        __syncthreads();
        for (int r = q; r < rows_here; r += 4) {
            const int64_t first = ((img_row0 + ch0 + r) * a.Wr + xlo) * 3;
            const int lead = (int)((base + (uintptr_t)first) & 3u);
            const uint8_t *src = reinterpret_cast<const uint8_t *>(&stage[r][0]) + lead + 3 * (xmin - xlo);
            int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
            for (int t = 0; t < xcnt; ++t) {
                const int k = hkl[t][c];
                s0 += k * (int)src[3 * t], s1 += k * (int)src[3 * t + 1], s2 += k * (int)src[3 * t + 2];
            }
            himg[ch0 + r][0][c] = (uint8_t)ig_clip8(s0);
            himg[ch0 + r][1][c] = (uint8_t)ig_clip8(s1);
            himg[ch0 + r][2][c] = (uint8_t)ig_clip8(s2);
        }
    }
    __syncthreads();
    if (!col_in)
        return;
    for (int i = 0; i < IG_TILE_H / 4; ++i) {
        const int oy = by * IG_TILE_H + q * (IG_TILE_H / 4) + i;
        if (oy >= a.fH)
            break;
        const int ymin = vb[2 * oy], ycnt = vb[2 * oy + 1];
        const int32_t *k = vk + (int64_t)oy * a.ks;
        int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
        for (int t = 0; t < ycnt; ++t) {
            const int w = k[t], r = ymin + t - r0;
            s0 += w * (int)himg[r][0][c], s1 += w * (int)himg[r][1][c], s2 += w * (int)himg[r][2][c];
        }
        const int v0 = ig_clip8(s0), v1 = ig_clip8(s1), v2 = ig_clip8(s2);
        if (a.kind == RAC_IG_F32_CHW) {
            float *o = (float *)out + (((int64_t)img * 3) * a.fH + oy) * a.fW + ox;
            const int64_t plane = (int64_t)a.fH * a.fW;
            o[0] = (float)v0, o[plane] = (float)v1, o[2 * plane] = (float)v2;
        } else {
            uint8_t *o = (uint8_t *)out + (((int64_t)img * a.fH + oy) * a.fW + ox) * 3;
            o[0] = (uint8_t)v0, o[1] = (uint8_t)v1, o[2] = (uint8_t)v2;
        }
    }
}

// One axis of one group's tables on the host: every position's taps inside [0, in_size) and inside its tile's span, every span inside
// the budget.  0, RAC_E_ARG or RAC_E_UNSUPPORTED (rac_last_error set).
static int ig_check_axis(const char *what, const char *axis, const int32_t *bounds, const int32_t *spans, int n, int tile, int in_size, int ks,
                         int budget)
{
    for (int i = 0; i < (n + tile - 1) / tile; ++i) {
        const int lo = spans[2 * i], hi = spans[2 * i + 1];
        RAC_CHECK_ARG(lo >= 0 && lo <= hi && hi <= in_size, "%s: %s tile %d spans [%d, %d) of a raw axis of %d", what, axis, i, lo, hi, in_size);
        if (hi - lo > budget) {
            rac_set_error("%s: %s tile %d reads %d raw positions, the kernel's LDS holds %d (the down-scale is too strong)", what, axis, i,
                          hi - lo, budget);
            return RAC_E_UNSUPPORTED;
        }
    }
    for (int o = 0; o < n; ++o) {
        const int first = bounds[2 * o], count = bounds[2 * o + 1], lo = spans[2 * (o / tile)], hi = spans[2 * (o / tile) + 1];
        RAC_CHECK_ARG(count >= 0 && count <= ks, "%s: %s %d has %d taps (0 .. %d)", what, axis, o, count, ks);
        RAC_CHECK_ARG(count == 0 || (first >= lo && first + count <= hi), "%s: %s %d reads [%d, %d), its tile spans [%d, %d)", what, axis, o,
                      first, first + count, lo, hi);
    }
    return 0;
}

extern "C" int rac_image_geom_fwd(const uint8_t *raw, const int32_t *tables, const int32_t *tables_host, void *out, int n_images, int group,
                                  int Hr, int Wr, int fH, int fW, int ksize, int out_kind, void *stream)
{
    const char *what = "rac_image_geom_fwd";
    RAC_CHECK_ARG(n_images >= 0 && group > 0 && n_images % group == 0, "%s: %d images in groups of %d", what, n_images, group);
    RAC_CHECK_ARG(Hr > 0 && Wr > 0 && fH > 0 && fW > 0 && ksize > 0, "%s: raw %d x %d, output %d x %d, %d taps", what, Hr, Wr, fH, fW, ksize);
    RAC_CHECK_ARG(out_kind == RAC_IG_F32_CHW || out_kind == RAC_IG_U8_HWC, "%s: out_kind %d", what, out_kind);
    RAC_CHECK_ARG(n_images == 0 || (raw && tables && tables_host && out), "%s: null pointer", what);
    RAC_CHECK_ARG(out_kind != RAC_IG_F32_CHW || (uintptr_t)out % 4 == 0, "%s: the float32 output is not 4-byte aligned", what);
    RAC_CHECK_ARG((uintptr_t)tables % 4 == 0, "%s: the tables are not 4-byte aligned", what);
    RAC_CHECK_ARG(n_images <= 65535 && (int64_t)fH * fW < ((int64_t)1 << 30) && (int64_t)Hr * Wr < ((int64_t)1 << 30),
                  "%s: %d images of %d x %d from %d x %d are too many", what, n_images, fH, fW, Hr, Wr);
    if (n_images == 0)
        return 0;
    if (ksize > IG_TAPS) {
        rac_set_error("%s: %d taps per position, the kernel holds %d (the down-scale is too strong)", what, ksize, IG_TAPS);
        return RAC_E_UNSUPPORTED;
    }
    IgArgs a;
    a.group = group, a.Hr = Hr, a.Wr = Wr, a.fH = fH, a.fW = fW, a.ks = ksize, a.kind = out_kind;
    a.ntx = (fW + IG_TILE_W - 1) / IG_TILE_W, a.nty = (fH + IG_TILE_H - 1) / IG_TILE_H;
    a.raw_bytes = (long long)n_images * Hr * Wr * 3;
    RAC_CHECK_ARG(a.nty <= 65535, "%s: %d output rows are too many", what, fH);
    const int64_t stride = 2 * (int64_t)fW + 2 * fH + 2 * a.ntx + 2 * a.nty + ((int64_t)fW + fH) * ksize;
    RAC_CHECK_ARG(stride * (n_images / group) < ((int64_t)1 << 31), "%s: the tables are too large", what);
    for (int g = 0; g < n_images / group; ++g) {
        const int32_t *hb = tables_host + g * stride, *vb = hb + 2 * fW, *tx = vb + 2 * fH, *ty = tx + 2 * a.ntx;
        int rc = ig_check_axis(what, "column", hb, tx, fW, IG_TILE_W, Wr, ksize, IG_SPAN_PX);
        if (rc == 0)
            rc = ig_check_axis(what, "row", vb, ty, fH, IG_TILE_H, Hr, ksize, IG_ROWS);
        if (rc != 0)
            return rc;
    }
    const dim3 grid((unsigned)a.ntx, (unsigned)a.nty, (unsigned)n_images), block(256);
    hipLaunchKernelGGL(ig_transform_kernel, grid, block, 0, (hipStream_t)stream, raw, tables, out, a);
    return rac_launch_status(what);
}
