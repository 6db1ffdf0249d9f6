// point_maps.hip -- point clouds to per-view maps on the device: the radar depth / RCS maps of RadarPointToMultiViewDepth and the lidar
// depth map of PointToMultiViewDepth (loaders/pipelines/loading.py:470-600), rules 1-6 of DESIGN 3.24.  gfx950, wave64.
//
// One projection routine (pm_project) serves every pass, so a value that is computed twice (the scatter pass and the resolve pass of
// the lidar map; the two scans of the radar kernel) has the same bits both times: float32, every operation rounded once, no
// contraction, IEEE division -- the order racformer_amd/point_maps.py restates in torch.
//
// Winners are chosen with 64-bit integer atomic min / max only.  A kept point's key is a non-negative float (lo > 0 is required), so
// its bit pattern orders as an unsigned integer.
//   lidar : per pixel  min of (key << 32 | index)                      -- the smallest (key, index)
//   radar : per column max of (cy << 52 | ~key << 20 | ~index & 0xfffff) -- the largest cy, there the smallest (key, index)
// Every output element is written by a resolve pass (pads as +0.0): no memset, no float atomics, nothing read back.
#include "rac_common.h"

#define PM_THREADS 256
#define PM_ROWS 8                    // rows per thread of the radar resolve pass (a column's value is the same in every row)
#define PM_EMPTY 0xffffffffffffffffull
typedef unsigned long long pm_u64;

struct PmView {
    float m[12];                     // rows 0..2 of lidar2img
};
struct PmGeom {
    float ds, wm, hm, lo, hi;        // downsample, map width / height (as floats: the reference compares floats), depth range
};

// Rules 1-3 for one point and one view.  false: dropped (NaN, inf and p_2 = 0 fail the comparisons).
__device__ __forceinline__ bool pm_project(const float *__restrict__ p, const PmView &v, const PmGeom &g, int &cx, int &cy, float &d,
                                           unsigned &key)
{
#pragma clang fp contract(off)
    const float x = p[0], y = p[1], z = p[2];
    // plain operators under the pragma above: the header's __fmul_rn / __fadd_rn are inline functions compiled under the default
    // contraction mode, and their products and sums fuse into v_fma_f32 once inlined (seen: depths one ulp off the restatement)
    const float p0 = x * v.m[0] + y * v.m[1] + z * v.m[2] + v.m[3];
    const float p1 = x * v.m[4] + y * v.m[5] + z * v.m[6] + v.m[7];
    const float p2 = x * v.m[8] + y * v.m[9] + z * v.m[10] + v.m[11];
    const float fx = rintf(__fdiv_rn(__fdiv_rn(p0, p2), g.ds)), fy = rintf(__fdiv_rn(__fdiv_rn(p1, p2), g.ds));      // half to even
    d = p2;
    if (!(fx >= 0.f && fx < g.wm && fy >= 0.f && fy < g.hm && p2 < g.hi && p2 >= g.lo))
        return false;
    cx = (int)fx;
    cy = (int)fy;
    const float rank = fx + fy * g.wm;
    const float k = rank + __fdiv_rn(p2, 100.f);
    key = __float_as_uint(k + 0.f);                      // (+ 0: a -0 key becomes +0)
    return true;
}

__device__ __forceinline__ PmView pm_load_view(const float *__restrict__ mats, int map)
{
    PmView v;
#pragma unroll
    for (int i = 0; i < 12; ++i)
        v.m[i] = mats[(size_t)map * 12 + i];
    return v;
}

// Four consecutive floats of one output row, from element `c0` on (c0 a multiple of 4 inside the row, the row `wp` wide): one 16-byte
// store where the address allows it, scalar stores otherwise and at the row's tail.
__device__ __forceinline__ void pm_store4(float *__restrict__ row, int c0, int wp, float a, float b, float c, float d)
{
    float *q = row + c0;
    if (c0 + 3 < wp && (reinterpret_cast<uintptr_t>(q) & 15u) == 0) {
        *reinterpret_cast<rac_f4 *>(q) = rac_f4{a, b, c, d};
        return;
    }
    const float v[4] = {a, b, c, d};
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (c0 + i < wp)
            q[i] = v[i];
}

// ------------------------------------------------------------------------------------------------ radar
// One workgroup per map (cloud, view).  scratch: per map `wm` winner words, then (after all maps' winner words) per map `wm` value
// words (depth bits | rcs bits << 32).  Phases, a workgroup barrier and a device-scope fence between them; the winner words are
// written and read with device-scope atomics only, so no phase reads a stale cache line:
//   0  the map's winner and value words = 0              (a kept point's word is never 0: ~key != 0 for a non-NaN key)
//   1  every kept point: max into its column's winner word
//   2  the same scan again, now with the running count of kept points (rule 5: the RCS written for a winner is that of the point at
//      the winner's POSITION AMONG THE KEPT POINTS); the one point whose word equals its column's winner word writes the value word
__global__ __launch_bounds__(PM_THREADS) void pm_radar_columns_kernel(const float *__restrict__ points, const int32_t *__restrict__ offsets,
                                                                     const float *__restrict__ mats, pm_u64 *__restrict__ scratch,
                                                                     int n_points, int n_views, int n_maps, int C, int rcs_col, int wm, PmGeom g)
{
    __shared__ int s_wave[PM_THREADS / RAC_WAVE];
    const int map = blockIdx.x, cloud = map / n_views, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = max(offsets[cloud], 0), n = min(offsets[cloud + 1], n_points) - base;      // (clamped: no read past the points)
    const PmView view = pm_load_view(mats, map);
    pm_u64 *win = scratch + (size_t)map * wm, *val = scratch + (size_t)n_maps * wm + (size_t)map * wm;

    for (int c = tid; c < wm; c += PM_THREADS) {
        __hip_atomic_store(win + c, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        val[c] = 0ull;
    }
    __threadfence();
    __syncthreads();

    for (int j0 = 0; j0 < n; j0 += PM_THREADS) {
        const int j = j0 + tid;
        int cx = 0, cy = 0;
        float d;
        unsigned key = 0;
        if (j < n && pm_project(points + (size_t)(base + j) * C, view, g, cx, cy, d, key)) {
            const pm_u64 word = ((pm_u64)cy << 52) | ((pm_u64)(~key) << 20) | (pm_u64)(~(unsigned)j & 0xfffffu);
            __hip_atomic_fetch_max(win + cx, word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __threadfence();
    __syncthreads();

    int running = 0;                                         // kept points before this chunk
    for (int j0 = 0; j0 < n; j0 += PM_THREADS) {
        const int j = j0 + tid;
        int cx = 0, cy = 0;
        float d = 0.f;
        unsigned key = 0;
        const bool kept = j < n && pm_project(points + (size_t)(base + j) * C, view, g, cx, cy, d, key);
        const pm_u64 ballot = __ballot(kept);
        if (lane == 0)
            s_wave[wave] = __popcll(ballot);
        __syncthreads();
        int before = running, total = running;
#pragma unroll
        for (int w = 0; w < PM_THREADS / RAC_WAVE; ++w) {
            before += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (kept) {
            const int s = before + __popcll(ballot & ((1ull << lane) - 1ull));        // position among the kept points, s <= j < n
            const pm_u64 word = ((pm_u64)cy << 52) | ((pm_u64)(~key) << 20) | (pm_u64)(~(unsigned)j & 0xfffffu);
            if (__hip_atomic_load(win + cx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == word)
                val[cx] = (pm_u64)__float_as_uint(d) | ((pm_u64)__float_as_uint(points[(size_t)(base + s) * C + rcs_col]) << 32);
        }
        running = total;
        __syncthreads();
    }
}

// Every element of the two maps: a column's value in rows < hm and columns < wm, +0.0 in the pads.  One thread: four columns of PM_ROWS rows.
__global__ __launch_bounds__(PM_THREADS) void pm_radar_fill_kernel(const pm_u64 *__restrict__ val, float *__restrict__ depth,
                                                                  float *__restrict__ rcs, int hm, int wm, int hp, int wp)
{
    const int quads = (wp + 3) >> 2, map = blockIdx.y;
    const int item = blockIdx.x * PM_THREADS + threadIdx.x, rg = item / quads, c0 = (item - rg * quads) * 4;
    if (rg * PM_ROWS >= hp)
        return;
    float dv[4], rv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const pm_u64 w = c0 + i < wm ? val[(size_t)map * wm + c0 + i] : 0ull;
        dv[i] = __uint_as_float((unsigned)w);
        rv[i] = __uint_as_float((unsigned)(w >> 32));
    }
    for (int r = rg * PM_ROWS; r < min(rg * PM_ROWS + PM_ROWS, hp); ++r) {
        const size_t row = ((size_t)map * hp + r) * wp;
        const bool in = r < hm;
        if (depth)
            pm_store4(depth + row, c0, wp, in ? dv[0] : 0.f, in ? dv[1] : 0.f, in ? dv[2] : 0.f, in ? dv[3] : 0.f);
        if (rcs)
            pm_store4(rcs + row, c0, wp, in ? rv[0] : 0.f, in ? rv[1] : 0.f, in ? rv[2] : 0.f, in ? rv[3] : 0.f);
    }
}

// ------------------------------------------------------------------------------------------------ lidar
__global__ __launch_bounds__(PM_THREADS) void pm_lidar_init_kernel(pm_u64 *__restrict__ scratch, size_t words)
{
    const size_t i = (size_t)blockIdx.x * PM_THREADS + threadIdx.x;
    if (i < words)
        scratch[i] = PM_EMPTY;
}

// grid (point chunks, views): the point's cloud from the offsets table, then min of (key, index in the cloud) into the pixel's word
__global__ __launch_bounds__(PM_THREADS) void pm_lidar_scatter_kernel(const float *__restrict__ points, const int32_t *__restrict__ offsets,
                                                                     const float *__restrict__ mats, pm_u64 *__restrict__ scratch,
                                                                     int n_points, int n_clouds, int n_views, int C, int hm, int wm, PmGeom g)
{
    const int i = blockIdx.x * PM_THREADS + threadIdx.x, viewi = blockIdx.y;
    if (i >= n_points)
        return;
    int lo = 0, hi = n_clouds;                               // the last cloud with offsets[cloud] <= i
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i)
            lo = mid;
        else
            hi = mid;
    }
    const int cloud = lo, j = i - offsets[cloud];
    if (j < 0 || i >= offsets[cloud + 1])                    // (a point no cloud owns: offsets that do not cover [0, n_points))
        return;
    const int map = cloud * n_views + viewi;
    const PmView view = pm_load_view(mats, map);
    int cx, cy;
    float d;
    unsigned key;
    if (pm_project(points + (size_t)i * C, view, g, cx, cy, d, key))
        atomicMin(scratch + ((size_t)map * hm + cy) * wm + cx, ((pm_u64)key << 32) | (unsigned)j);
}

// Every element of the map: the winner's depth, recomputed by the same routine (the same bits), 0 where no point fell, +0.0 in the pads.
__global__ __launch_bounds__(PM_THREADS) void pm_lidar_resolve_kernel(const float *__restrict__ points, const int32_t *__restrict__ offsets,
                                                                     const float *__restrict__ mats, const pm_u64 *__restrict__ scratch,
                                                                     float *__restrict__ out, int n_views, int C, int hm, int wm, int hp,
                                                                     int wp, PmGeom g)
{
    const int quads = (wp + 3) >> 2, map = blockIdx.y;
    const int item = blockIdx.x * PM_THREADS + threadIdx.x, r = item / quads, c0 = (item - r * quads) * 4;
    if (r >= hp)
        return;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < hm) {
        const int base = offsets[map / n_views];
        const PmView view = pm_load_view(mats, map);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (c0 + i >= wm)
                continue;
            const pm_u64 w = scratch[((size_t)map * hm + r) * wm + c0 + i];
            if (w == PM_EMPTY)
                continue;
            int cx, cy;
            unsigned key;
            pm_project(points + (size_t)(base + (int)(unsigned)w) * C, view, g, cx, cy, v[i], key);
        }
    }
    pm_store4(out + ((size_t)map * hp + r) * wp, c0, wp, v[0], v[1], v[2], v[3]);
}

// ------------------------------------------------------------------------------------------------ C-ABI
static int pm_args(const char *what, const void *points, const void *offsets, const void *mats, const void *scratch, int n_points, int n_clouds,
                   int n_views, int C, int H, int W, int Hp, int Wp, int ds, float lo, float hi, int64_t scratch_words, int64_t need_words)
{
    RAC_CHECK_ARG(points && offsets && mats && scratch, "%s: null pointer", what);
    RAC_CHECK_ARG(n_points >= 0 && n_clouds >= 1 && n_views >= 1 && C >= 3, "%s: n_points=%d n_clouds=%d n_views=%d C=%d", what, n_points,
                  n_clouds, n_views, C);
    RAC_CHECK_ARG(ds >= 1, "%s: ds=%d (at least 1)", what, ds);
    RAC_CHECK_ARG(H >= ds && W >= ds, "%s: a %d x %d image has no map at ds=%d", what, H, W, ds);
    RAC_CHECK_ARG(Hp >= H / ds && Wp >= W / ds, "%s: the padded map %d x %d is smaller than the map %d x %d", what, Hp, Wp, H / ds, W / ds);
    RAC_CHECK_ARG(lo == lo && hi == hi, "%s: depth range [%g, %g)", what, lo, hi);
    RAC_CHECK_ARG(((uintptr_t)points & 3) == 0 && ((uintptr_t)offsets & 3) == 0 && ((uintptr_t)mats & 3) == 0 && ((uintptr_t)scratch & 7) == 0,
                  "%s: misaligned pointer (4 bytes; 8 for the scratch)", what);
    if ((int64_t)(H / ds) * (W / ds) > ((int64_t)1 << 18) || hi > 99.f || !(lo > 0.f)) {
        rac_set_error("%s: a %d x %d map with depths in [%g, %g): beyond 2^18 pixels, hi = 99 or with lo <= 0 the float32 sort key no "
                      "longer orders the pixels as the reference does", what, H / ds, W / ds, lo, hi);
        return RAC_E_UNSUPPORTED;
    }
    if (n_points >= (1 << 20) || H / ds > 4096) {
        rac_set_error("%s: %d points / %d map rows (clouds below 2^20 points, at most 4096 rows)", what, n_points, H / ds);
        return RAC_E_UNSUPPORTED;
    }
    RAC_CHECK_ARG((int64_t)n_clouds * n_views <= 65535, "%s: %d x %d maps are too many (65535)", what, n_clouds, n_views);
    RAC_CHECK_ARG((int64_t)n_clouds * n_views * Hp * ((Wp + 3) / 4) < ((int64_t)1 << 31), "%s: the maps are too large", what);
    RAC_CHECK_ARG(scratch_words >= need_words, "%s: scratch of %lld words, %lld needed", what, (long long)scratch_words, (long long)need_words);
    return 0;
}

extern "C" int rac_point_maps_radar_fwd(const float *points, const int32_t *cloud_offsets, const float *mats, float *radar_depth, float *radar_rcs,
                                        uint64_t *scratch, int64_t scratch_words, int n_points, int n_clouds, int n_views, int C, int rcs_col, int H,
                                        int W, int Hp, int Wp, int ds, float lo, float hi, void *stream)
{
    const char *what = "rac_point_maps_radar_fwd";
    RAC_CHECK_ARG(radar_depth || radar_rcs, "%s: null pointer (neither a depth nor an RCS map)", what);
    RAC_CHECK_ARG(((uintptr_t)radar_depth & 3) == 0 && ((uintptr_t)radar_rcs & 3) == 0, "%s: misaligned output", what);
    RAC_CHECK_ARG(rcs_col >= 0 && rcs_col < C, "%s: RCS column %d outside [0, %d)", what, rcs_col, C);
    const int64_t need = ds >= 1 ? 2 * (int64_t)n_clouds * n_views * (W / ds) : 0;
    if (int rc = pm_args(what, points, cloud_offsets, mats, scratch, n_points, n_clouds, n_views, C, H, W, Hp, Wp, ds, lo, hi, scratch_words, need))
        return rc;
    const int hm = H / ds, wm = W / ds, n_maps = n_clouds * n_views;
    const PmGeom g = {(float)ds, (float)wm, (float)hm, lo, hi};
    hipLaunchKernelGGL(pm_radar_columns_kernel, dim3(n_maps), dim3(PM_THREADS), 0, (hipStream_t)stream, points, cloud_offsets, mats,
                       (pm_u64 *)scratch, n_points, n_views, n_maps, C, rcs_col, wm, g);
    const int items = ((Hp + PM_ROWS - 1) / PM_ROWS) * ((Wp + 3) / 4);
    hipLaunchKernelGGL(pm_radar_fill_kernel, dim3((items + PM_THREADS - 1) / PM_THREADS, n_maps), dim3(PM_THREADS), 0, (hipStream_t)stream,
                       (const pm_u64 *)scratch + (size_t)n_maps * wm, radar_depth, radar_rcs, hm, wm, Hp, Wp);
    return rac_launch_status(what);
}

extern "C" int rac_point_maps_lidar_fwd(const float *points, const int32_t *cloud_offsets, const float *mats, float *gt_depth, uint64_t *scratch,
                                        int64_t scratch_words, int n_points, int n_clouds, int n_views, int C, int H, int W, int Hp, int Wp, int ds,
                                        float lo, float hi, void *stream)
{
    const char *what = "rac_point_maps_lidar_fwd";
    RAC_CHECK_ARG(gt_depth && ((uintptr_t)gt_depth & 3) == 0, "%s: null or misaligned output", what);
    const int64_t need = ds >= 1 ? (int64_t)n_clouds * n_views * (H / ds) * (W / ds) : 0;
    if (int rc = pm_args(what, points, cloud_offsets, mats, scratch, n_points, n_clouds, n_views, C, H, W, Hp, Wp, ds, lo, hi, scratch_words, need))
        return rc;
    const int hm = H / ds, wm = W / ds, n_maps = n_clouds * n_views;
    const PmGeom g = {(float)ds, (float)wm, (float)hm, lo, hi};
    hipLaunchKernelGGL(pm_lidar_init_kernel, dim3((unsigned)((need + PM_THREADS - 1) / PM_THREADS)), dim3(PM_THREADS), 0, (hipStream_t)stream,
                       (pm_u64 *)scratch, (size_t)need);
    if (n_points > 0)
        hipLaunchKernelGGL(pm_lidar_scatter_kernel, dim3((n_points + PM_THREADS - 1) / PM_THREADS, n_views), dim3(PM_THREADS), 0,
                           (hipStream_t)stream, points, cloud_offsets, mats, (pm_u64 *)scratch, n_points, n_clouds, n_views, C, hm, wm, g);
    const int items = Hp * ((Wp + 3) / 4);
    hipLaunchKernelGGL(pm_lidar_resolve_kernel, dim3((items + PM_THREADS - 1) / PM_THREADS, n_maps), dim3(PM_THREADS), 0, (hipStream_t)stream,
                       points, cloud_offsets, mats, (const pm_u64 *)scratch, gt_depth, n_views, C, hm, wm, Hp, Wp, g);
    return rac_launch_status(what);
}
