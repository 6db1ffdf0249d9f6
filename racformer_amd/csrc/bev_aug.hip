// bev_aug.hip -- the scene's rotation about z and isotropic scaling on the device: what RaCGlobalRotScaleTransImage
// (loaders/pipelines/transforms.py:398-464) does to the lidar cloud, the radar clouds and the ground-truth boxes, the rules of
// DESIGN 3.26, for all samples of a step in one launch.  gfx950, wave64.
//
// The unit of work is a CHUNK: RAC_BEV_CHUNK consecutive rows of ONE segment (a segment's last chunk is short), one workgroup per
// chunk, one row per lane.  The host tables (rac_bev_seg, rac_bev_chunk) say which; rac_bev_aug_fwd checks their host copies before
// it launches, so a lane touches only rows a segment names.  A lane reads its whole row into registers, then writes it: dst == src
// works in place.  Accesses are scalar on purpose: rows are 5, 7 or 9 floats, so consecutive rows are 20, 28 or 36 bytes apart and only
// every fourth one starts on a 16-byte boundary -- a wide path would be lane-divergent, and the launch moves about 2 MB: it is bound
// by its latency, not by the memory system.  A wave's loads of one column fall into the same cache lines as its loads of the next.
//
// cos and sin come from the host (the draws table): no trigonometric function is evaluated here.  float32, every operation rounded
// once, no contraction -- the order racformer_amd/bev_aug.py restates in torch, and the products by 0 are kept (no fast-math flag
// allows the compiler to drop them): they carry a NaN or inf coordinate into the other two as the reference's matmul does.
#include "rac_common.h"

#define BA_THREADS RAC_BEV_CHUNK
static_assert(BA_THREADS % RAC_WAVE == 0, "a chunk is a whole number of waves");

// The segments' pointers come out of a device table, so the compiler cannot tell their address space and would emit flat accesses; they
// are global memory by the entry's contract, and this cast says so.
#define BA_GLOBAL __attribute__((address_space(1)))

struct BaDraw {
    float c, s, a, r;
};

// x, y, z of a point or of a box's bottom centre.
__device__ __forceinline__ void ba_rotate_scale(float &x, float &y, float &z, const BaDraw &d)
{
#pragma clang fp contract(off)
    // plain operators under the pragma above (the header's __fmul_rn / __fadd_rn fuse once inlined: csrc/point_maps.hip)
    const float ns = -d.s;
    const float x1 = ((x * d.c + y * ns) + z * 0.f) * d.r;
    const float y1 = ((x * d.s + y * d.c) + z * 0.f) * d.r;
    const float z1 = ((x * 0.f + y * 0.f) + z * 1.f) * d.r;
    x = x1;
    y = y1;
    z = z1;
}

// w, l, h, yaw and (nine columns) vx, vy of a box.
__device__ __forceinline__ void ba_box_rest(float &w, float &l, float &h, float &yaw, float &vx, float &vy, const BaDraw &d)
{
#pragma clang fp contract(off)
    const float ns = -d.s;
    w = w * d.r;
    l = l * d.r;
    h = h * d.r;
    yaw = yaw + d.a;
    const float vx1 = (vx * d.c + vy * ns) * d.r;
    const float vy1 = (vx * d.s + vy * d.c) * d.r;
    vx = vx1;
    vy = vy1;
}

__global__ __launch_bounds__(BA_THREADS) void bev_aug_kernel(const rac_bev_seg *__restrict__ segs, const rac_bev_chunk *__restrict__ chunks,
                                                             const float *__restrict__ draws)
{
    const rac_bev_chunk ch = chunks[blockIdx.x];
    const rac_bev_seg sg = segs[ch.seg];
    const int row = ch.row0 + (int)threadIdx.x, C = sg.cols;
    if (row >= sg.rows)
        return;
    // (bits, not floats: the columns that are only copied keep every NaN payload; src and dst may be the same memory: no __restrict__)
    const BA_GLOBAL unsigned *src = (const BA_GLOBAL unsigned *)sg.src + (size_t)row * C;
    BA_GLOBAL unsigned *dst = (BA_GLOBAL unsigned *)sg.dst + (size_t)row * C;
    const float *__restrict__ dr = draws + 4 * (size_t)sg.sample;
    const BaDraw d = {dr[0], dr[1], dr[2], dr[3]};

    unsigned v[RAC_BEV_MAX_COLS];
#pragma unroll
    for (int k = 0; k < RAC_BEV_MAX_COLS; ++k)
        v[k] = k < C ? src[k] : 0u;

    float x = __uint_as_float(v[0]), y = __uint_as_float(v[1]), z = __uint_as_float(v[2]);
    ba_rotate_scale(x, y, z, d);
    v[0] = __float_as_uint(x);
    v[1] = __float_as_uint(y);
    v[2] = __float_as_uint(z);
    if (sg.kind == RAC_BEV_BOXES) {
        float w = __uint_as_float(v[3]), l = __uint_as_float(v[4]), h = __uint_as_float(v[5]), yaw = __uint_as_float(v[6]);
        float vx = __uint_as_float(v[7]), vy = __uint_as_float(v[8]);           // (0 in a seven-column box, and not written back)
        ba_box_rest(w, l, h, yaw, vx, vy, d);
        v[3] = __float_as_uint(w);
        v[4] = __float_as_uint(l);
        v[5] = __float_as_uint(h);
        v[6] = __float_as_uint(yaw);
        v[7] = __float_as_uint(vx);
        v[8] = __float_as_uint(vy);
    }

#pragma unroll
    for (int k = 0; k < RAC_BEV_MAX_COLS; ++k)
        if (k < C)
            dst[k] = v[k];
}

// [lo, hi) of a segment's bytes on one side
static inline void ba_span(const void *p, const rac_bev_seg &s, uintptr_t &lo, uintptr_t &hi)
{
    lo = (uintptr_t)p;
    hi = lo + (uintptr_t)s.rows * (uintptr_t)s.cols * sizeof(float);
}

extern "C" int rac_bev_aug_fwd(const rac_bev_seg *segs, const rac_bev_chunk *chunks, const rac_bev_seg *segs_host, const rac_bev_chunk *chunks_host,
                               const float *draws, int n_segs, int n_chunks, int n_samples, void *stream)
{
    const char *what = "rac_bev_aug_fwd";
    RAC_CHECK_ARG(segs && chunks && segs_host && chunks_host && draws, "%s: null pointer", what);
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(segs) | reinterpret_cast<uintptr_t>(segs_host)) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(chunks) | reinterpret_cast<uintptr_t>(chunks_host) | reinterpret_cast<uintptr_t>(draws)) & 3) == 0,
                  "%s: misaligned table (8 bytes for the segments, 4 for the chunks and the draws)", what);
    RAC_CHECK_ARG(n_segs >= 1 && n_segs <= 1024 && n_chunks >= 0 && n_samples >= 1, "%s: n_segs=%d (1..1024) n_chunks=%d n_samples=%d", what,
                  n_segs, n_chunks, n_samples);
    int chunk = 0;
    for (int i = 0; i < n_segs; ++i) {
        const rac_bev_seg &s = segs_host[i];
        RAC_CHECK_ARG(s.kind == RAC_BEV_POINTS || s.kind == RAC_BEV_BOXES, "%s: segment %d: kind=%d", what, i, s.kind);
        RAC_CHECK_ARG(s.kind == RAC_BEV_POINTS ? (s.cols >= 3 && s.cols <= RAC_BEV_MAX_COLS) : (s.cols == 7 || s.cols == 9),
                      "%s: segment %d: %d columns (points: 3..%d, boxes: 7 or 9)", what, i, s.cols, RAC_BEV_MAX_COLS);
        RAC_CHECK_ARG(s.rows >= 0 && (int64_t)s.rows * s.cols < ((int64_t)1 << 31), "%s: segment %d: rows=%d", what, i, s.rows);
        RAC_CHECK_ARG(s.sample >= 0 && s.sample < n_samples, "%s: segment %d: sample %d outside [0, %d)", what, i, s.sample, n_samples);
        if (s.rows == 0)
            continue;
        RAC_CHECK_ARG(s.src && s.dst && ((reinterpret_cast<uintptr_t>(s.src) | reinterpret_cast<uintptr_t>(s.dst)) & 3) == 0,
                      "%s: segment %d: null or misaligned rows", what, i);
        uintptr_t dlo, dhi, lo, hi;
        ba_span(s.dst, s, dlo, dhi);
        for (int j = 0; j < n_segs; ++j) {
            const rac_bev_seg &o = segs_host[j];
            if (o.rows == 0)
                continue;
            ba_span(o.src, o, lo, hi);
            RAC_CHECK_ARG(dhi <= lo || hi <= dlo || (i == j && s.dst == s.src), "%s: segment %d's destination overlaps segment %d's source", what, i, j);
            ba_span(o.dst, o, lo, hi);
            RAC_CHECK_ARG(i == j || dhi <= lo || hi <= dlo, "%s: the destinations of segments %d and %d overlap", what, i, j);
        }
        for (int row0 = 0; row0 < s.rows; row0 += RAC_BEV_CHUNK, ++chunk)
            RAC_CHECK_ARG(chunk < n_chunks && chunks_host[chunk].seg == i && chunks_host[chunk].row0 == row0,
                          "%s: chunk %d is not rows %d.. of segment %d", what, chunk, row0, i);
    }
    RAC_CHECK_ARG(chunk == n_chunks, "%s: %d chunks for segments of %d", what, n_chunks, chunk);
    if (n_chunks == 0)
        return 0;
    hipLaunchKernelGGL(bev_aug_kernel, dim3((unsigned)n_chunks), dim3(BA_THREADS), 0, (hipStream_t)stream, segs, chunks, draws);
    return rac_launch_status(what);
}
