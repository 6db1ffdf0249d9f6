// radar_pillars.hip -- the radar branch in front of the decoder's radar BEV stack (models/racformer.py:130-177 extract_pts_feat /
// radar_voxelize; mmcv's hard Voxelization, mmdet3d's PillarFeatureNet and PointPillarsScatter), gfx950.
//
// All clouds of a call arrive packed: points [n_points][C] f32 and cloud_offsets [n_clouds + 1]; cloud c owns the rows
// [offsets[c], offsets[c + 1]).  Every launch is sized by n_points or n_clouds * cells, the pillar counts stay on the device, the
// only atomics are integer min / max (whose result does not depend on the order): capturable and bitwise reproducible.
//
// Hard voxelization, the sequential definition (mmcv's CPU path, its deterministic=True) from parallel kernels:
//   * key(p) = cloud * cells + cell(p), or -1 for a point outside the range;   first[key] = min p          (rp_cells_kernel)
//   * a point is its cell's FIRST iff first[key(p)] == p; the cell's pillar index is the number of earlier firsts of the cloud
//     (one workgroup per cloud: ballot / popcount scan over the cloud's points in order); the max_voxels cap applies to that
//     rank -- a cell whose first point comes after the cap never gets a pillar, later points of registered cells still do
//                                                                                                           (rp_rank_kernel)
//   * a point's slot is the number of earlier points with the same key (256-key tiles through LDS, every thread compares its
//     key with the tile's: broadcast reads); slot < max_num_points keeps it                                 (rp_slots_kernel)
//     This is n^2 / 2 compares per cloud -- 1.1 M for a 1500-point radar sweep, microseconds; a lidar-sized cloud would want
//     the sort of lss_view.hip's table builder instead.
// Pillar rows of cloud c are packed at the cloud's own offset (a cloud has at most as many pillars as points), padding rows
// are defined: voxels 0, coors -1, num_points 0.
#include "rac_common.h"

#define RP_MAX_C 16
#define RP_FEAT 64

struct RpGeom {
    float lo[3], vs[3];      // x, y, z
    int grid[3];
};

__device__ __forceinline__ int rp_clamp_off(const int32_t *__restrict__ off, int c, int n_points) { return min(max(off[c], 0), n_points); }

// the cloud of row p: the last c with offsets[c] <= p (empty clouds share an offset with their successor), -1 past the last cloud
__device__ __forceinline__ int rp_cloud_of(const int32_t *__restrict__ off, int n_clouds, int p)
{
    if (p >= off[n_clouds] || p < off[0])
        return -1;
    int lo = 0, hi = n_clouds;       // invariant: off[lo] <= p < off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void rp_init_kernel(uint32_t *__restrict__ first, int32_t *__restrict__ cellpillar, long n_tab,
                                                      float *__restrict__ voxels, long n_vox, int32_t *__restrict__ coors,
                                                      int32_t *__restrict__ num_points, long n_points, int32_t *__restrict__ counts,
                                                      int n_clouds, uint32_t *__restrict__ amax)
{
    const long stride = (long)gridDim.x * 256, t0 = (long)blockIdx.x * 256 + threadIdx.x;
    for (long i = t0; i < n_tab; i += stride) {
        first[i] = 0xffffffffu;
        cellpillar[i] = -1;
    }
    for (long i = t0; i < n_vox; i += stride)
        voxels[i] = 0.f;
    for (long i = t0; i < n_points; i += stride) {
        coors[4 * i + 0] = -1;
        coors[4 * i + 1] = -1;
        coors[4 * i + 2] = -1;
        coors[4 * i + 3] = -1;
        num_points[i] = 0;
    }
    for (long i = t0; i < n_clouds; i += stride)
        counts[i] = 0;
    if (t0 == 0)
        *amax = 0u;
}

// c_j = floor((p_j - lo_j) / vs_j) in IEEE f32 (one subtraction, one correctly rounded division: NOT a reciprocal multiply, which
// moves 13 of the 129 cell edges k * 0.8f of the f8 grid); kept iff 0 <= c_j < grid_j on all three axes (a NaN fails the test).
__global__ __launch_bounds__(256) void rp_cells_kernel(const float *__restrict__ points, const int32_t *__restrict__ off, int n_points,
                                                       int n_clouds, int C, const RpGeom g, int32_t *__restrict__ key,
                                                       uint32_t *__restrict__ first, uint32_t *__restrict__ amax)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    unsigned mx = 0u;
    if (p < n_points) {
        const int cloud = rp_cloud_of(off, n_clouds, p);
        int k = -1;
        if (cloud >= 0) {
            const float *v = points + (size_t)p * C;
            float c[3];
            bool in = true;
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                c[j] = floorf(__fdiv_rn(__fsub_rn(v[j], g.lo[j]), g.vs[j]));
                in = in && c[j] >= 0.f && c[j] < (float)g.grid[j];
            }
            if (in) {
                k = cloud * (g.grid[0] * g.grid[1] * g.grid[2]) + ((int)c[2] * g.grid[1] + (int)c[1]) * g.grid[0] + (int)c[0];
                atomicMin(first + k, (uint32_t)p);
                for (int j = 0; j < C; ++j)
                    mx = max(mx, rac_absbits(v[j]));
            }
        }
        key[p] = k;
    }
    // max |value| over the kept points (bit patterns of |x|: monotonic, integer max -- order-free)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        mx = max(mx, (unsigned)__shfl_xor((int)mx, o));
    if ((threadIdx.x & 63) == 0 && mx != 0u)
        atomicMax(amax, mx);
}

// One workgroup per cloud: the cloud's points in order, 1024 at a time; rank of a first point = firsts before it.
__global__ __launch_bounds__(1024) void rp_rank_kernel(const int32_t *__restrict__ off, int n_points, const int32_t *__restrict__ key,
                                                       const uint32_t *__restrict__ first, int cells, int gx, int gy, int max_voxels,
                                                       int32_t *__restrict__ cellpillar, int32_t *__restrict__ coors,
                                                       int32_t *__restrict__ counts)
{
    __shared__ int s_wave[16];
    const int c = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int begin = rp_clamp_off(off, c, n_points), end = max(begin, rp_clamp_off(off, c + 1, n_points));
    int running = 0;
    for (int base = begin; base < end; base += 1024) {
        const int p = base + t;
        int k = -1;
        bool flag = false;
        if (p < end) {
            k = key[p];
            flag = k >= 0 && k / cells == c && first[k] == (uint32_t)p;
        }
        const unsigned long long b = __ballot(flag);
        const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
        if (lane == 0)
            s_wave[wave] = __popcll(b);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int n = s_wave[w];
            before += w < wave ? n : 0;
            total += n;
        }
        const int rank = running + before + in_wave;
        if (flag && rank < max_voxels) {
            const int cell = k - c * cells, cx = cell % gx, cy = (cell / gx) % gy, cz = cell / (gx * gy);
            cellpillar[k] = rank;
            int32_t *o = coors + 4 * (size_t)(begin + rank);       // rank < firsts of this cloud <= end - begin
            o[0] = c;
            o[1] = cz;
            o[2] = cy;
            o[3] = cx;
        }
        running += total;
        __syncthreads();
    }
    if (t == 0)
        counts[c] = min(running, max_voxels);
}

__global__ __launch_bounds__(256) void rp_slots_kernel(const float *__restrict__ points, const int32_t *__restrict__ off, int n_points,
                                                       int n_clouds, int C, int cells, const int32_t *__restrict__ key,
                                                       const int32_t *__restrict__ cellpillar, int max_num_points,
                                                       float *__restrict__ voxels, int32_t *__restrict__ num_points)
{
    __shared__ int s_key[256];
    const int t = threadIdx.x, p0 = blockIdx.x * 256, p = p0 + t;
    const int mykey = p < n_points ? key[p] : -1;
    // earlier points of the same cell lie in the same cloud: scan from the start of the cloud of this block's first point
    const int c0 = rp_cloud_of(off, n_clouds, p0);
    const int j0 = c0 >= 0 ? rp_clamp_off(off, c0, n_points) : p0;
    const int j1 = min(p0 + 256, n_points);
    int cnt = 0;
    for (int tile = j0; tile < j1; tile += 256) {
        s_key[t] = tile + t < j1 ? key[tile + t] : -1;
        __syncthreads();
        if (mykey >= 0) {
            const int lim = p - tile;                   // compare with points tile + i < p
#pragma unroll 8
            for (int i = 0; i < 256; ++i)
                cnt += (s_key[i] == mykey) & (i < lim);
        }
        __syncthreads();
    }
    if (mykey < 0)
        return;
    const int pil = cellpillar[mykey];
    if (pil < 0 || cnt >= max_num_points)
        return;
    const int row = rp_clamp_off(off, mykey / cells, n_points) + pil;
    const float *src = points + (size_t)p * C;
    float *dst = voxels + ((size_t)row * max_num_points + cnt) * C;
    for (int j = 0; j < C; ++j)
        dst[j] = src[j];
    atomicMax(num_points + row, cnt + 1);
}

// ------------------------------------------------------------------------------------------------ pillar encode + scatter
__global__ __launch_bounds__(256) void rp_fill_zero_kernel(uint4 *__restrict__ dst, long n)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        dst[i] = make_uint4(0u, 0u, 0u, 0u);
}

struct RpEncode {
    const float *voxels;
    const int32_t *coors, *num_points;
    const float *wt, *shift, *amax;
    float bound_mul, bound_add;
    float *canvas, *feats;
    _Float16 *image;
    int n_rows, n_clouds, C, P, H, W;
    float vs[3], center0[3];
};

// The pillar decoration, shared by the inference kernel and the training kernels below.  Every operand is wave-uniform.
// rp_pillar_centres: the mean of the pillar's points (the padded rows add zeros, as in the reference's sum over dim 1) and the cell's
// centre, x / y / z from coors columns 3 / 2 / 1.
__device__ __forceinline__ void rp_pillar_centres(const float *__restrict__ vox, int P, int C, int np, const int32_t *__restrict__ co,
                                                  const float (&vs)[3], const float (&center0)[3], float (&mean)[3], float (&centre)[3])
{
#pragma clang fp contract(off)
    float sum[3] = {0.f, 0.f, 0.f};
    for (int s = 0; s < P; ++s)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            sum[j] += vox[s * C + j];
    const int cc[3] = {co[3], co[2], co[1]};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        mean[j] = __fdiv_rn(sum[j], (float)np);
        centre[j] = (float)cc[j] * vs[j] + center0[j];
    }
}

// one point row -> its decorated features: raw [C] (zero past C), then [xyz - mean | xyz - cell centre]
__device__ __forceinline__ void rp_row_features(const float *__restrict__ v, int C, const float (&mean)[3], const float (&centre)[3],
                                                float (&f)[RP_MAX_C], float (&fc)[6])
{
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < RP_MAX_C; ++k)
        f[k] = k < C ? v[k] : 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        fc[j] = f[j] - mean[j];
        fc[3 + j] = f[j] - centre[j];
    }
}

// W f of one point row for the lane's channel: an fma chain in ascending feature order
__device__ __forceinline__ float rp_row_dot(const float *__restrict__ v, int C, const float (&w)[RP_MAX_C], const float (&wc)[6],
                                            const float (&mean)[3], const float (&centre)[3])
{
    float f[RP_MAX_C], fc[6];
    rp_row_features(v, C, mean, centre, f, fc);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < RP_MAX_C; ++k)
        if (k < C)
            acc = __builtin_fmaf(w[k], f[k], acc);
#pragma unroll
    for (int j = 0; j < 6; ++j)
        acc = __builtin_fmaf(wc[j], fc[j], acc);
    return acc;
}

// the lane's column of the transposed Linear weight wt [C + 6][64]
__device__ __forceinline__ void rp_load_weight(const float *__restrict__ wt, int C, int ch, float (&w)[RP_MAX_C], float (&wc)[6])
{
#pragma unroll
    for (int k = 0; k < RP_MAX_C; ++k)
        w[k] = k < C ? wt[k * RP_FEAT + ch] : 0.f;
#pragma unroll
    for (int j = 0; j < 6; ++j)
        wc[j] = wt[(C + j) * RP_FEAT + ch];
}

// One wave per pillar row, a lane per output channel.  PillarFeatureNet (legacy=False, with_cluster_center, with_voxel_center):
// features = [raw C | xyz - mean | xyz - cell centre]; y = relu(W' f + shift) with the BatchNorm folded into W' and shift; max over
// the max_num_points rows, the padded rows taking part with relu(shift) (the reference multiplies their features by 0 and still
// feeds them through Linear / BN / ReLU / max).  Every operand of the decoration is wave-uniform; the dot product runs in
// ascending feature order (fma chain).
__global__ __launch_bounds__(256) void rp_encode_kernel(const RpEncode a)
{
#pragma clang fp contract(off)
    const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), ch = threadIdx.x & 63;
    if (r >= a.n_rows)
        return;
    const int32_t *co = a.coors + 4 * (size_t)r;
    const int cloud = co[0], cy = co[2], cx = co[3];
    const int np = a.num_points[r];
    if (cloud < 0 || np <= 0)
        return;
    const bool on_map = cloud < a.n_clouds && cy >= 0 && cy < a.H && cx >= 0 && cx < a.W;   // (foreign coors never write outside)
    const int C = a.C;
    float w[RP_MAX_C], wc[6];
    rp_load_weight(a.wt, C, ch, w, wc);
    const float shift = a.shift[ch];
    const float *vox = a.voxels + (size_t)r * a.P * C;
    float mean[3], centre[3];
    rp_pillar_centres(vox, a.P, C, np, co, a.vs, a.center0, mean, centre);
    // (every candidate is >= 0: 0 is neutral for the max; a NaN among the candidates wins, as torch.max has it)
    float best = np < a.P ? rac_relu(shift) : 0.f;
    for (int s = 0; s < min(np, a.P); ++s) {
        const float y = rac_relu(rp_row_dot(vox + s * C, C, w, wc, mean, centre) + shift);
        if (y > best || y != y)
            best = y;
    }
    if (a.feats)
        a.feats[(size_t)r * RP_FEAT + ch] = best;
    if (a.canvas && on_map)
        a.canvas[(((size_t)cloud * RP_FEAT + ch) * a.H + cy) * a.W + cx] = best;
    if (a.image && on_map) {
        const float so = rac_act_scale((a.amax ? a.bound_mul * *a.amax : 0.f) + a.bound_add);
        const size_t pix = ((size_t)cloud * (a.H + 2) + cy + 1) * (a.W + 2) + cx + 1;
        _Float16 *d = a.image + (pix * (RP_FEAT / 32) + (ch >> 5)) * 64 + (ch & 31);
        _Float16 hi, lo;
        rac_split_f16(best * so, hi, lo);
        d[0] = hi;
        d[32] = lo;
    }
}

static unsigned rp_blocks(long n, long cap = 4096)
{
    long b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

extern "C" int rac_pillar_voxelize_fwd(const float *points, const int32_t *cloud_offsets, float *voxels, int32_t *coors,
                                       int32_t *num_points, int32_t *counts, float *amax, int32_t *workspace, int n_points, int n_clouds,
                                       int C, float lo_x, float lo_y, float lo_z, float vs_x, float vs_y, float vs_z, int grid_x,
                                       int grid_y, int grid_z, int max_num_points, int max_voxels, void *stream)
{
    RAC_CHECK_ARG(n_points >= 0 && n_clouds >= 0, "rac_pillar_voxelize_fwd: n_points=%d n_clouds=%d", n_points, n_clouds);
    RAC_CHECK_ARG(C >= 4 && C <= RP_MAX_C, "rac_pillar_voxelize_fwd: point width C=%d (4..%d)", C, RP_MAX_C);
    RAC_CHECK_ARG(max_num_points >= 1 && max_num_points <= 32 && max_voxels >= 1,
                  "rac_pillar_voxelize_fwd: max_num_points=%d (1..32) max_voxels=%d (>= 1)", max_num_points, max_voxels);
    RAC_CHECK_ARG(grid_x > 0 && grid_y > 0 && grid_z > 0 && vs_x > 0.f && vs_y > 0.f && vs_z > 0.f,
                  "rac_pillar_voxelize_fwd: grid %d x %d x %d, voxel size %g x %g x %g", grid_x, grid_y, grid_z, vs_x, vs_y, vs_z);
    const int64_t cells = (int64_t)grid_x * grid_y * grid_z;
    RAC_CHECK_ARG(cells * (n_clouds > 0 ? n_clouds : 1) < ((int64_t)1 << 30) && (int64_t)n_points * max_num_points * C < ((int64_t)1 << 31),
                  "rac_pillar_voxelize_fwd: %d clouds x %lld cells / %d points exceed the int32 tables", n_clouds, (long long)cells,
                  n_points);
    if (n_clouds == 0)
        return 0;
    RAC_CHECK_ARG(cloud_offsets && counts && amax && workspace && (n_points == 0 || (points && voxels && coors && num_points)),
                  "rac_pillar_voxelize_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const long n_tab = cells * n_clouds;
    uint32_t *first = reinterpret_cast<uint32_t *>(workspace);
    int32_t *cellpillar = workspace + n_tab, *key = workspace + 2 * n_tab;
    const RpGeom g = {{lo_x, lo_y, lo_z}, {vs_x, vs_y, vs_z}, {grid_x, grid_y, grid_z}};
    const long n_vox = (long)n_points * max_num_points * C;
    hipLaunchKernelGGL(rp_init_kernel, dim3(rp_blocks(n_tab > n_vox ? n_tab : n_vox)), dim3(256), 0, st, first, cellpillar, n_tab, voxels,
                       n_vox, coors, num_points, (long)n_points, counts, n_clouds, reinterpret_cast<uint32_t *>(amax));
    if (n_points > 0)
        hipLaunchKernelGGL(rp_cells_kernel, dim3((n_points + 255) / 256), dim3(256), 0, st, points, cloud_offsets, n_points, n_clouds, C, g,
                           key, first, reinterpret_cast<uint32_t *>(amax));
    hipLaunchKernelGGL(rp_rank_kernel, dim3(n_clouds), dim3(1024), 0, st, cloud_offsets, n_points, key, first, (int)cells, grid_x, grid_y,
                       max_voxels, cellpillar, coors, counts);
    if (n_points > 0)
        hipLaunchKernelGGL(rp_slots_kernel, dim3((n_points + 255) / 256), dim3(256), 0, st, points, cloud_offsets, n_points, n_clouds, C,
                           (int)cells, key, cellpillar, max_num_points, voxels, num_points);
    return rac_launch_status("rac_pillar_voxelize_fwd");
}

extern "C" int rac_pillar_encode_fwd(const float *voxels, const int32_t *coors, const int32_t *num_points, const float *wt,
                                     const float *shift, const float *amax, float bound_mul, float bound_add, float *canvas, void *image,
                                     float *feats, int n_rows, int n_clouds, int C, int max_num_points, int F, float vs_x, float vs_y, float vs_z,
                                     float center_x, float center_y, float center_z, int H, int W, void *stream)
{
    RAC_CHECK_ARG(n_rows >= 0 && n_clouds >= 0 && H > 0 && W > 0, "rac_pillar_encode_fwd: n_rows=%d n_clouds=%d H=%d W=%d", n_rows, n_clouds, H,
                  W);
    RAC_CHECK_ARG(C >= 4 && C <= RP_MAX_C && max_num_points >= 1 && max_num_points <= 32,
                  "rac_pillar_encode_fwd: point width C=%d (4..%d), max_num_points=%d (1..32)", C, RP_MAX_C, max_num_points);
    RAC_CHECK_ARG(F == RP_FEAT, "rac_pillar_encode_fwd: built for %d feature channels, got %d", RP_FEAT, F);
    RAC_CHECK_ARG(bound_mul >= 0.f && bound_add >= 0.f, "rac_pillar_encode_fwd: scale constants must be >= 0");
    RAC_CHECK_ARG((int64_t)n_clouds * (H + 2) * (W + 2) < ((int64_t)1 << 31) / RP_FEAT, "rac_pillar_encode_fwd: %d maps of %d x %d are too large",
                  n_clouds, H, W);
    if (n_clouds == 0)
        return 0;
    RAC_CHECK_ARG(canvas || image || feats, "rac_pillar_encode_fwd: no destination (canvas, image and feats are all null)");
    RAC_CHECK_ARG(wt && shift && (n_rows == 0 || (voxels && coors && num_points)), "rac_pillar_encode_fwd: null pointer");
    RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(canvas) | reinterpret_cast<uintptr_t>(image)) & 15) == 0,
                  "rac_pillar_encode_fwd: canvas / image must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    // cells without a pillar read as zero on every call: both destinations are cleared on the stream first (the image's border with it)
    if (canvas) {
        const long n = (long)n_clouds * RP_FEAT * H * W / 4;
        hipLaunchKernelGGL(rp_fill_zero_kernel, dim3(rp_blocks(n, 8192)), dim3(256), 0, st, reinterpret_cast<uint4 *>(canvas), n);
    }
    if (image) {
        const long n = (long)n_clouds * (H + 2) * (W + 2) * (RP_FEAT * 4 / 16);
        hipLaunchKernelGGL(rp_fill_zero_kernel, dim3(rp_blocks(n, 8192)), dim3(256), 0, st, reinterpret_cast<uint4 *>(image), n);
    }
    if (n_rows > 0) {
        RpEncode a;
        a.voxels = voxels; a.coors = coors; a.num_points = num_points; a.wt = wt; a.shift = shift; a.amax = amax;
        a.bound_mul = bound_mul; a.bound_add = bound_add; a.canvas = canvas; a.feats = feats; a.image = reinterpret_cast<_Float16 *>(image);
        a.n_rows = n_rows; a.n_clouds = n_clouds; a.C = C; a.P = max_num_points; a.H = H; a.W = W;
        a.vs[0] = vs_x; a.vs[1] = vs_y; a.vs[2] = vs_z; a.center0[0] = center_x; a.center0[1] = center_y; a.center0[2] = center_z;
        hipLaunchKernelGGL(rp_encode_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, st, a);
    }
    return rac_launch_status("rac_pillar_encode_fwd");
}

// ------------------------------------------------------------------------------------------------ the PFN layer in training mode
// Linear (no bias) -> BatchNorm1d on BATCH statistics -> ReLU -> max over the P slots -> scatter, and its backward.  The statistics of
// a channel run over all n = M * P rows of the call (M = the real pillar rows, counted on the device from num_points; never read
// back); the padded rows are exactly 0 and add nothing to the sums, so only real rows are touched and n alone knows about the rest.
// x = W f of every real row is kept in xbuf [n_rows][P][64] for the apply pass and the backward.
// Sums: float64 (sum x, sum x^2 as in batchnorm_train.hip); a pillar's rows in slot order, the pillars of one of 16 contiguous row
// ranges in ascending order, the 16 ranges in ascending order -- a function of n_rows alone.  No float atomics.
// The winning slot of a (pillar, channel) is the FIRST maximum (a padded slot comes after the real ones and is saved as -1).  torch
// may pick another of several tied slots; tied rows are identical inputs (duplicate radar returns), all padded, or both at the ReLU's
// zero, and in each case every parameter gradient is the same.
#define RP_SUM_GROUPS 16
#define RP_DW_ROWS 64            // pillar rows per workgroup of the dW kernel: 4 waves x 16 rows

struct RpTrain {
    const float *voxels;
    const int32_t *coors, *num_points;
    const float *wt, *gamma, *beta;
    float *running_mean, *running_var;
    int64_t *tracked;
    float *xbuf, *stat, *feats, *canvas;
    double *part;
    int32_t *n_total, *slots;
    int n_rows, n_clouds, C, P, H, W;
    float vs[3], center0[3];
    float eps, momentum;
};

__device__ __forceinline__ bool rp_row_valid(const int32_t *__restrict__ coors, const int32_t *__restrict__ num_points, int r)
{
    return coors[4 * (size_t)r] >= 0 && num_points[r] > 0;
}

// x = W f of the real rows; part[r] = (sum x [64], sum x^2 [64]) of pillar r, zeros for a padding row
__global__ __launch_bounds__(256) void rp_train_x_kernel(const RpTrain a)
{
    const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), ch = threadIdx.x & 63;
    if (r >= a.n_rows)
        return;
    double s1 = 0.0, s2 = 0.0;
    if (rp_row_valid(a.coors, a.num_points, r)) {
        const int C = a.C, np = min(a.num_points[r], a.P);
        float w[RP_MAX_C], wc[6], mean[3], centre[3];
        rp_load_weight(a.wt, C, ch, w, wc);
        const float *vox = a.voxels + (size_t)r * a.P * C;
        rp_pillar_centres(vox, a.P, C, a.num_points[r], a.coors + 4 * (size_t)r, a.vs, a.center0, mean, centre);
        for (int s = 0; s < np; ++s) {
            const float x = rp_row_dot(vox + s * C, C, w, wc, mean, centre);
            a.xbuf[((size_t)r * a.P + s) * RP_FEAT + ch] = x;
            s1 += (double)x;
            s2 += (double)x * (double)x;
        }
    }
    a.part[((size_t)r * 2 + 0) * RP_FEAT + ch] = s1;
    a.part[((size_t)r * 2 + 1) * RP_FEAT + ch] = s2;
}

// One workgroup: out[0 / 1][ch] = the two sums of part over all rows in the fixed order of the section comment, *m_out = the number
// of real rows.  Every thread returns with the totals of its channel.
__device__ __forceinline__ void rp_sum_rows(const double *__restrict__ part, const int32_t *__restrict__ coors,
                                            const int32_t *__restrict__ num_points, int n_rows, double &s1, double &s2, int &m)
{
    __shared__ double sh[2][RP_SUM_GROUPS][RP_FEAT];
    __shared__ int sh_m[RP_SUM_GROUPS];
    const int grp = threadIdx.x >> 6, ch = threadIdx.x & 63;
    const int per = (n_rows + RP_SUM_GROUPS - 1) / RP_SUM_GROUPS, r0 = grp * per, r1 = min(n_rows, r0 + per);
    double a1 = 0.0, a2 = 0.0;
    int cnt = 0;
    for (int r = r0; r < r1; ++r) {
        a1 += part[((size_t)r * 2 + 0) * RP_FEAT + ch];
        a2 += part[((size_t)r * 2 + 1) * RP_FEAT + ch];
        cnt += rp_row_valid(coors, num_points, r) ? 1 : 0;
    }
    sh[0][grp][ch] = a1;
    sh[1][grp][ch] = a2;
    if (ch == 0)
        sh_m[grp] = cnt;
    __syncthreads();
    s1 = 0.0;
    s2 = 0.0;
    m = 0;
#pragma unroll
    for (int k = 0; k < RP_SUM_GROUPS; ++k) {
        s1 += sh[0][k][ch];
        s2 += sh[1][k][ch];
        m += sh_m[k];
    }
}

// stat = [mean 64 | invstd 64], *n_total = M * P; the BatchNorm1d running statistics as nn.BatchNorm1d updates them in training mode.
// No pillar at all: stat = 0, n_total = 0, the running statistics stay as they are.
__global__ __launch_bounds__(1024) void rp_train_stats_kernel(const RpTrain a)
{
    double s1, s2;
    int m;
    rp_sum_rows(a.part, a.coors, a.num_points, a.n_rows, s1, s2, m);
    if (threadIdx.x >= RP_FEAT)
        return;
    const int ch = threadIdx.x;
    if (ch == 0)
        *a.n_total = m * a.P;
    if (m == 0) {
        a.stat[ch] = 0.f;
        a.stat[RP_FEAT + ch] = 0.f;
        return;
    }
    const double n = (double)m * (double)a.P, mu = s1 / n;
    double var = s2 / n - mu * mu;
    var = var > 0.0 ? var : (var == var ? 0.0 : var);
    a.stat[ch] = (float)mu;
    a.stat[RP_FEAT + ch] = (float)(1.0 / sqrt(var + (double)a.eps));
    if (a.running_mean) {
        const double mo = (double)a.momentum;
        a.running_mean[ch] = (float)((1.0 - mo) * (double)a.running_mean[ch] + mo * mu);
        a.running_var[ch] = (float)((1.0 - mo) * (double)a.running_var[ch] + mo * (var * (n / (n - 1.0))));
        if (ch == 0)
            *a.tracked += 1;
    }
}

__device__ __forceinline__ float rp_bn_relu(float x, float m, float is, float g, float b)
{
#pragma clang fp contract(off)
    return rac_relu(((x - m) * is) * g + b);
}

// BatchNorm + ReLU + max over the slots (first maximum), the winner and its slot saved, the canvas cell written
__global__ __launch_bounds__(256) void rp_train_apply_kernel(const RpTrain a)
{
    const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), ch = threadIdx.x & 63;
    if (r >= a.n_rows)
        return;
    float best = 0.f;
    int slot = -1;
    if (rp_row_valid(a.coors, a.num_points, r)) {
        const int np = min(a.num_points[r], a.P);
        const float m = a.stat[ch], is = a.stat[RP_FEAT + ch], g = a.gamma[ch], b = a.beta[ch];
        const float *x = a.xbuf + (size_t)r * a.P * RP_FEAT + ch;
        best = rp_bn_relu(x[0], m, is, g, b);
        slot = 0;
        for (int s = 1; s < np; ++s) {
            const float y = rp_bn_relu(x[s * RP_FEAT], m, is, g, b);
            if (y > best || y != y) {     // (a NaN wins, as torch.max has it; which slot it leaves is unspecified)
                best = y;
                slot = s;
            }
        }
        if (np < a.P) {
            const float y = rp_bn_relu(0.f, m, is, g, b);
            if (y > best || y != y) {
                best = y;
                slot = -1;
            }
        }
        const int32_t *co = a.coors + 4 * (size_t)r;
        const int cloud = co[0], cy = co[2], cx = co[3];
        if (cloud < a.n_clouds && cy >= 0 && cy < a.H && cx >= 0 && cx < a.W)
            a.canvas[(((size_t)cloud * RP_FEAT + ch) * a.H + cy) * a.W + cx] = best;
    }
    a.feats[(size_t)r * RP_FEAT + ch] = best;
    a.slots[(size_t)r * RP_FEAT + ch] = slot;
}

struct RpTrainBwd {
    const float *dcanvas, *voxels;
    const int32_t *coors, *num_points;
    const float *gamma, *xbuf, *stat, *feats;
    const int32_t *n_total, *slots;
    double *part, *dwpart;
    float *dw, *dgamma, *dbeta;
    int n_rows, n_clouds, C, P, H, W, n_blocks;
    float vs[3], center0[3];
};

// the canvas gradient of (pillar r, channel ch) behind the ReLU: 0 for a padding row, a cell off the map or a winner at 0
__device__ __forceinline__ float rp_gm(const RpTrainBwd &a, int r, int ch)
{
    if (!rp_row_valid(a.coors, a.num_points, r))
        return 0.f;
    const int32_t *co = a.coors + 4 * (size_t)r;
    const int cloud = co[0], cy = co[2], cx = co[3];
    if (!(cloud < a.n_clouds && cy >= 0 && cy < a.H && cx >= 0 && cx < a.W) || !(a.feats[(size_t)r * RP_FEAT + ch] > 0.f))
        return 0.f;
    return a.dcanvas[(((size_t)cloud * RP_FEAT + ch) * a.H + cy) * a.W + cx];
}

// part[r] = (gm [64], gm * xhat of the winning slot [64]) of pillar r
__global__ __launch_bounds__(256) void rp_train_bwd_rows_kernel(const RpTrainBwd a)
{
#pragma clang fp contract(off)
    const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), ch = threadIdx.x & 63;
    if (r >= a.n_rows)
        return;
    const float gm = rp_gm(a, r, ch);
    double p = 0.0;
    if (gm != 0.f) {
        const int slot = a.slots[(size_t)r * RP_FEAT + ch];
        const float xw = slot >= 0 ? a.xbuf[((size_t)r * a.P + slot) * RP_FEAT + ch] : 0.f;
        p = (double)gm * (double)((xw - a.stat[ch]) * a.stat[RP_FEAT + ch]);
    }
    a.part[((size_t)r * 2 + 0) * RP_FEAT + ch] = (double)gm;
    a.part[((size_t)r * 2 + 1) * RP_FEAT + ch] = p;
}

__global__ __launch_bounds__(1024) void rp_train_bwd_finish_kernel(const RpTrainBwd a)
{
    double s1, s2;
    int m;
    rp_sum_rows(a.part, a.coors, a.num_points, a.n_rows, s1, s2, m);
    if (threadIdx.x < RP_FEAT) {
        a.dbeta[threadIdx.x] = (float)s1;
        a.dgamma[threadIdx.x] = (float)s2;
    }
}

// dwpart[block][k][ch] = sum over the block's pillar rows and their real slots of dx[row][ch] * f[row][k],
// dx = gamma * invstd * (gm [winning slot] - dbeta / n - xhat * dgamma / n).  A wave takes 16 rows in ascending order, the four waves
// are added in ascending order.
__global__ __launch_bounds__(256) void rp_train_bwd_dw_kernel(const RpTrainBwd a)
{
#pragma clang fp contract(off)
    __shared__ double sh[3][RP_MAX_C + 6][RP_FEAT];
    const int wave = threadIdx.x >> 6, ch = threadIdx.x & 63, C = a.C;
    const int n = *a.n_total;
    const float inv_n = n > 0 ? (float)(1.0 / (double)n) : 0.f;
    const float m = a.stat[ch], is = a.stat[RP_FEAT + ch], k = a.gamma[ch] * is, cb = a.dbeta[ch] * inv_n, cg = a.dgamma[ch] * inv_n;
    double acc[RP_MAX_C], accc[6];
#pragma unroll
    for (int j = 0; j < RP_MAX_C; ++j)
        acc[j] = 0.0;
#pragma unroll
    for (int j = 0; j < 6; ++j)
        accc[j] = 0.0;
    for (int i = 0; i < RP_DW_ROWS / 4; ++i) {
        const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * RP_DW_ROWS + wave * (RP_DW_ROWS / 4) + i);
        if (r >= a.n_rows || !rp_row_valid(a.coors, a.num_points, r))
            continue;
        const int np = min(a.num_points[r], a.P);
        const float gm = rp_gm(a, r, ch);
        const int slot = a.slots[(size_t)r * RP_FEAT + ch];
        const float *vox = a.voxels + (size_t)r * a.P * C;
        float mean[3], centre[3];
        rp_pillar_centres(vox, a.P, C, a.num_points[r], a.coors + 4 * (size_t)r, a.vs, a.center0, mean, centre);
        for (int s = 0; s < np; ++s) {
            float f[RP_MAX_C], fc[6];
            rp_row_features(vox + s * C, C, mean, centre, f, fc);
            const float xh = (a.xbuf[((size_t)r * a.P + s) * RP_FEAT + ch] - m) * is;
            const float dx = k * (((s == slot ? gm : 0.f) - cb) - xh * cg);
#pragma unroll
            for (int j = 0; j < RP_MAX_C; ++j)
                if (j < C)
                    acc[j] += (double)dx * (double)f[j];
#pragma unroll
            for (int j = 0; j < 6; ++j)
                accc[j] += (double)dx * (double)fc[j];
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int j = 0; j < RP_MAX_C; ++j)
            sh[wave - 1][j][ch] = acc[j];
#pragma unroll
        for (int j = 0; j < 6; ++j)
            sh[wave - 1][RP_MAX_C + j][ch] = accc[j];
    }
    __syncthreads();
    if (wave > 0)
        return;
    double *out = a.dwpart + (size_t)blockIdx.x * (C + 6) * RP_FEAT;
#pragma unroll
    for (int j = 0; j < RP_MAX_C; ++j)
        if (j < C)
            out[j * RP_FEAT + ch] = ((acc[j] + sh[0][j][ch]) + sh[1][j][ch]) + sh[2][j][ch];
#pragma unroll
    for (int j = 0; j < 6; ++j)
        out[(C + j) * RP_FEAT + ch] = ((accc[j] + sh[0][RP_MAX_C + j][ch]) + sh[1][RP_MAX_C + j][ch]) + sh[2][RP_MAX_C + j][ch];
}

// dw [64][C + 6] = the blocks' partial sums in ascending order
__global__ __launch_bounds__(64) void rp_train_bwd_dw_finish_kernel(const RpTrainBwd a)
{
    const int kf = blockIdx.x, ch = threadIdx.x, F = a.C + 6;
    double s = 0.0;
    for (int b = 0; b < a.n_blocks; ++b)
        s += a.dwpart[((size_t)b * F + kf) * RP_FEAT + ch];
    a.dw[ch * F + kf] = (float)s;
}

static int rp_train_check(const char *what, int n_rows, int n_clouds, int C, int P, int F, int H, int W)
{
    RAC_CHECK_ARG(n_rows >= 0 && n_clouds >= 1 && H > 0 && W > 0, "%s: n_rows=%d n_clouds=%d H=%d W=%d", what, n_rows, n_clouds, H, W);
    RAC_CHECK_ARG(C >= 4 && C <= RP_MAX_C && P >= 2 && P <= 32, "%s: point width C=%d (4..%d), max_num_points=%d (2..32: one pillar has to "
                  "give the batch statistics two rows)", what, C, RP_MAX_C, P);
    RAC_CHECK_ARG(F == RP_FEAT, "%s: built for %d feature channels, got %d", what, RP_FEAT, F);
    RAC_CHECK_ARG((int64_t)n_clouds * H * W < ((int64_t)1 << 31) / RP_FEAT && (int64_t)n_rows * P < ((int64_t)1 << 31) / RP_FEAT,
                  "%s: %d maps of %d x %d / %d rows are too large", what, n_clouds, H, W, n_rows);
    return 0;
}

extern "C" int rac_pillar_train_fwd(const float *voxels, const int32_t *coors, const int32_t *num_points, const float *wt,
                                    const float *gamma, const float *beta, float *running_mean, float *running_var,
                                    int64_t *num_batches_tracked, float *xbuf, double *workspace, float *stat, int32_t *n_total,
                                    float *feats, int32_t *slots, float *canvas, int n_rows, int n_clouds, int C, int max_num_points,
                                    int F, float eps, float momentum, float vs_x, float vs_y, float vs_z, float center_x, float center_y,
                                    float center_z, int H, int W, void *stream)
{
    if (int rc = rp_train_check("rac_pillar_train_fwd", n_rows, n_clouds, C, max_num_points, F, H, W))
        return rc;
    RAC_CHECK_ARG(wt && gamma && beta && stat && n_total && canvas && workspace, "rac_pillar_train_fwd: null pointer");
    RAC_CHECK_ARG(n_rows == 0 || (voxels && coors && num_points && xbuf && feats && slots), "rac_pillar_train_fwd: null pointer");
    RAC_CHECK_ARG((running_mean && running_var && num_batches_tracked) || (!running_mean && !running_var && !num_batches_tracked),
                  "rac_pillar_train_fwd: running_mean, running_var and num_batches_tracked are given together or not at all");
    RAC_CHECK_ARG(eps >= 0.f && momentum >= 0.f && momentum <= 1.f, "rac_pillar_train_fwd: eps=%g momentum=%g", eps, momentum);
    RAC_CHECK_ARG((reinterpret_cast<uintptr_t>(canvas) & 15) == 0, "rac_pillar_train_fwd: canvas must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    RpTrain a;
    a.voxels = voxels; a.coors = coors; a.num_points = num_points; a.wt = wt; a.gamma = gamma; a.beta = beta;
    a.running_mean = running_mean; a.running_var = running_var; a.tracked = num_batches_tracked;
    a.xbuf = xbuf; a.stat = stat; a.feats = feats; a.canvas = canvas; a.part = workspace; a.n_total = n_total; a.slots = slots;
    a.n_rows = n_rows; a.n_clouds = n_clouds; a.C = C; a.P = max_num_points; a.H = H; a.W = W;
    a.vs[0] = vs_x; a.vs[1] = vs_y; a.vs[2] = vs_z; a.center0[0] = center_x; a.center0[1] = center_y; a.center0[2] = center_z;
    a.eps = eps; a.momentum = momentum;
    const long n4 = (long)n_clouds * RP_FEAT * H * W / 4;
    hipLaunchKernelGGL(rp_fill_zero_kernel, dim3(rp_blocks(n4, 8192)), dim3(256), 0, st, reinterpret_cast<uint4 *>(canvas), n4);
    if (n_rows > 0)
        hipLaunchKernelGGL(rp_train_x_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rp_train_stats_kernel, dim3(1), dim3(1024), 0, st, a);
    if (n_rows > 0)
        hipLaunchKernelGGL(rp_train_apply_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, st, a);
    return rac_launch_status("rac_pillar_train_fwd");
}

extern "C" int rac_pillar_train_bwd(const float *dcanvas, const float *voxels, const int32_t *coors, const int32_t *num_points,
                                    const float *gamma, const float *xbuf, const float *stat, const int32_t *n_total, const float *feats,
                                    const int32_t *slots, double *workspace, float *dw, float *dgamma, float *dbeta, int n_rows,
                                    int n_clouds, int C, int max_num_points, int F, float vs_x, float vs_y, float vs_z, float center_x,
                                    float center_y, float center_z, int H, int W, void *stream)
{
    if (int rc = rp_train_check("rac_pillar_train_bwd", n_rows, n_clouds, C, max_num_points, F, H, W))
        return rc;
    RAC_CHECK_ARG(dcanvas && gamma && stat && n_total && workspace && dgamma && dbeta, "rac_pillar_train_bwd: null pointer");
    RAC_CHECK_ARG(n_rows == 0 || (voxels && coors && num_points && xbuf && feats && slots), "rac_pillar_train_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    RpTrainBwd a;
    a.dcanvas = dcanvas; a.voxels = voxels; a.coors = coors; a.num_points = num_points; a.gamma = gamma; a.xbuf = xbuf; a.stat = stat;
    a.feats = feats; a.n_total = n_total; a.slots = slots; a.part = workspace; a.dwpart = workspace + (size_t)n_rows * 2 * RP_FEAT;
    a.dw = dw; a.dgamma = dgamma; a.dbeta = dbeta;
    a.n_rows = n_rows; a.n_clouds = n_clouds; a.C = C; a.P = max_num_points; a.H = H; a.W = W;
    a.n_blocks = (n_rows + RP_DW_ROWS - 1) / RP_DW_ROWS;
    a.vs[0] = vs_x; a.vs[1] = vs_y; a.vs[2] = vs_z; a.center0[0] = center_x; a.center0[1] = center_y; a.center0[2] = center_z;
    if (n_rows > 0)
        hipLaunchKernelGGL(rp_train_bwd_rows_kernel, dim3((n_rows + 3) / 4), dim3(256), 0, st, a);
    hipLaunchKernelGGL(rp_train_bwd_finish_kernel, dim3(1), dim3(1024), 0, st, a);
    if (dw) {
        if (n_rows > 0)
            hipLaunchKernelGGL(rp_train_bwd_dw_kernel, dim3(a.n_blocks), dim3(256), 0, st, a);
        hipLaunchKernelGGL(rp_train_bwd_dw_finish_kernel, dim3(C + 6), dim3(64), 0, st, a);
    }
    return rac_launch_status("rac_pillar_train_bwd");
}
