// lss_view.hip -- the Lift-Splat view transform around the splat (frustum -> BEV), forward and backward, for gfx950.
//
// Replaces the view-transform half of LSSViewTransformer_racformer (models/necks/view_transformer_racformer.py):
//   get_lidar_coor (:112-153)            -> rac_lss_cells_fwd   : one thread per frustum point, its BEV cell or -1
//   voxel_pooling_prepare_v2 (:202-260)  -> rac_lss_tables_fwd  : the five rank / interval tables and two counts, on the device
//   view_transform_core (:268-295)       -> rac_lss_softmax_stats_fwd + rac_lss_splat_fwd (softmax applied on the fly)
//   its autograd backward                -> rac_lss_view_bwd    : pixel-major gather, one writer per element
// rac_lss_transpose_fwd is the layout pass between the reference's channel-first tensors and the channel-last rows the gathers read.
//
// Nothing here is sized by a count read back: every launch covers an upper bound (points, cells) and the kernels read the two
// device counts themselves, so the whole operator can be captured into a graph.  Integer atomics build the histogram and the
// unordered fill; no floating-point value is accumulated atomically and every sum has a fixed order (bitwise reproducible).
#include "rac_common.h"

#define LSS_CHUNK 64     // points per splat chunk (one wave walks one chunk)
#define LSS_RUN 16       // consecutive x cells a combine workgroup stages through LDS
#define LSS_MAX_C 320
#define LSS_MAX_D 256

__device__ __forceinline__ int lss_lane_i(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ float lss_lane_f(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// ------------------------------------------------------------------------------------------------------------ cells
// grid (ceil(HW / 256), D, B*N): the matrix and the depth value are uniform per workgroup (scalar loads).
__global__ __launch_bounds__(256) void lss_cells_kernel(const float *__restrict__ img2lidar, const float *__restrict__ depth_tab,
                                                        const float *__restrict__ v_tab, const float *__restrict__ u_tab,
                                                        int32_t *__restrict__ cells, int N, int D, int H, int W, float lx, float ly,
                                                        float lz, float ix, float iy, float iz, int X, int Y, int Z)
{
    const int bn = blockIdx.z, d = blockIdx.y;
    const int hw = blockIdx.x * 256 + threadIdx.x;
    if (hw >= H * W)
        return;
    const float *m = img2lidar + (size_t)bn * 16;
    const float dv = depth_tab[d];
    const float s = fmaxf(dv, 1e-5f);
    const float a = u_tab[hw % W] * s, b = v_tab[hw / W] * s;
    // M . (a, b, d, 1), first three rows
    const float px = fmaf(m[0], a, fmaf(m[1], b, fmaf(m[2], dv, m[3])));
    const float py = fmaf(m[4], a, fmaf(m[5], b, fmaf(m[6], dv, m[7])));
    const float pz = fmaf(m[8], a, fmaf(m[9], b, fmaf(m[10], dv, m[11])));
    // true float32 division, truncation toward zero: a scaled coordinate in (-1, 0) lands in cell 0 and is kept (the reference's
    // .long()); the test in the float domain is the same predicate as 0 <= trunc(s) < size and is false for NaN
    const float sx = __fdiv_rn(px - lx, ix), sy = __fdiv_rn(py - ly, iy), sz = __fdiv_rn(pz - lz, iz);
    const bool kept = sx > -1.f && sx < (float)X && sy > -1.f && sy < (float)Y && sz > -1.f && sz < (float)Z;
    int cell = -1;
    if (kept)
        cell = (((bn / N) * Z + (int)sz) * Y + (int)sy) * X + (int)sx;
    cells[((size_t)bn * D + d) * (size_t)(H * W) + hw] = cell;
}

// ------------------------------------------------------------------------------------------------------------ tables
// Scratch words are reset by a kernel, not by hipMemsetAsync: a captured plan then holds kernel nodes only (memset nodes inside
// instantiated graphs have misbehaved on this runtime).
__global__ __launch_bounds__(256) void lss_fill_i32_kernel(int32_t *__restrict__ p, int n, int32_t value)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n)
        p[i] = value;
}

__global__ __launch_bounds__(256) void lss_hist_kernel(const int32_t *__restrict__ cells, int n_points, int32_t *__restrict__ count)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_points)
        return;
    const int c = cells[p];
    if (c >= 0)
        atomicAdd(count + c, 1);
}

// One workgroup: exclusive scans over the cells of (points, occupied) -> cell_start, the interval tables, the two counts, and
// the interval tables' padding (start 0, length 0).
__global__ __launch_bounds__(1024) void lss_scan_kernel(const int32_t *__restrict__ count, int n_cells, int n_int_max,
                                                        int32_t *__restrict__ cell_start, int32_t *__restrict__ interval_starts,
                                                        int32_t *__restrict__ interval_lengths, int32_t *__restrict__ counts)
{
    __shared__ int s_pts[1024], s_occ[1024];
    const int t = threadIdx.x;
    const int per = (n_cells + 1023) / 1024;
    const int c0 = min(t * per, n_cells), c1 = min(c0 + per, n_cells);
    int pts = 0, occ = 0;
    for (int c = c0; c < c1; ++c) {
        const int k = count[c];
        pts += k;
        occ += k > 0;
    }
    s_pts[t] = pts;
    s_occ[t] = occ;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int a = t >= off ? s_pts[t - off] : 0, b = t >= off ? s_occ[t - off] : 0;
        __syncthreads();
        s_pts[t] += a;
        s_occ[t] += b;
        __syncthreads();
    }
    int start = s_pts[t] - pts, iv = s_occ[t] - occ;
    const int n_kept = s_pts[1023], n_int = s_occ[1023];
    for (int c = c0; c < c1; ++c) {
        const int k = count[c];
        cell_start[c] = start;
        if (k > 0) {
            interval_starts[iv] = start;
            interval_lengths[iv] = k;
            ++iv;
        }
        start += k;
    }
    for (int i = n_int + t; i < n_int_max; i += 1024) {
        interval_starts[i] = 0;
        interval_lengths[i] = 0;
    }
    if (t == 0) {
        counts[0] = n_kept;
        counts[1] = n_int;
    }
}

// unordered fill: the points of a cell into the cell's slots, in arrival order
__global__ __launch_bounds__(256) void lss_fill_kernel(const int32_t *__restrict__ cells, int n_points,
                                                       const int32_t *__restrict__ cell_start, int32_t *__restrict__ cursor,
                                                       int32_t *__restrict__ slots)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_points)
        return;
    const int c = cells[p];
    if (c >= 0)
        slots[cell_start[c] + atomicAdd(cursor + c, 1)] = p;
}

// The per-cell order: slot j's point goes to the position given by the number of smaller point indices in its cell (the indices
// are distinct), i.e. ascending ranks_depth inside a cell whatever order the fill arrived in.  Slots past the kept count are padding (-1).
__global__ __launch_bounds__(256) void lss_order_kernel(const int32_t *__restrict__ cells, const int32_t *__restrict__ slots,
                                                        const int32_t *__restrict__ cell_start, const int32_t *__restrict__ count,
                                                        const int32_t *__restrict__ counts, int n_points, int D, int HW,
                                                        int32_t *__restrict__ ranks_bev, int32_t *__restrict__ ranks_depth,
                                                        int32_t *__restrict__ ranks_feat)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n_points)
        return;
    const int n_kept = counts[0];
    if (j < n_kept) {
        const int v = slots[j];
        const int c = cells[v];
        const int start = cell_start[c], len = count[c];
        const int32_t *s = slots + start;
        int rank = 0;
        for (int i = 0; i < len; ++i)
            rank += s[i] < v;
        ranks_depth[start + rank] = v;
        ranks_feat[start + rank] = (v / (D * HW)) * HW + v % HW;
        ranks_bev[start + rank] = c;
    } else {
        // (positions >= n_kept are written by nobody else: the kept points fill exactly [0, n_kept))
        ranks_depth[j] = -1;
        ranks_feat[j] = -1;
        ranks_bev[j] = -1;
    }
}

// ------------------------------------------------------------------------------------------------------------ softmax statistics
// One thread per pixel: running max and sum over the D logits (stride HW, coalesced across the threads); stats[pixel] = (max, 1 / sum).
__global__ __launch_bounds__(64) void lss_softmax_stats_kernel(const float *__restrict__ logits, float2 *__restrict__ stats, int npix,
                                                               int D, int HW)
{
    const int pix = blockIdx.x * 64 + threadIdx.x;
    if (pix >= npix)
        return;
    const float *p = logits + (size_t)(pix / HW) * D * HW + pix % HW;
    float mx = p[0];
    for (int d = 1; d < D; ++d)
        mx = fmaxf(mx, p[(size_t)d * HW]);
    double sum = 0.0;                                  // (D adds per pixel: the double sum costs nothing and rounds once)
    for (int d = 0; d < D; ++d)
        sum += (double)expf(p[(size_t)d * HW] - mx);
    stats[pix] = make_float2(mx, (float)(1.0 / sum));
}

// ------------------------------------------------------------------------------------------------------------ transposition
// dst[n][l][r] = src[n][r][l], r < rows, l < cols; 32 x 32 tiles through LDS, both sides coalesced.
__global__ __launch_bounds__(256) void lss_transpose_kernel(const float *__restrict__ src, float *__restrict__ dst, int rows, int cols)
{
    __shared__ float tile[32][33];
    const float *s = src + (size_t)blockIdx.z * rows * cols;
    float *d = dst + (size_t)blockIdx.z * rows * cols;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int l0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int k = ty; k < 32; k += 8)
        if (r0 + k < rows && l0 + tx < cols)
            tile[k][tx] = s[(size_t)(r0 + k) * cols + l0 + tx];
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
        if (l0 + k < cols && r0 + tx < rows)
            d[(size_t)(l0 + k) * rows + r0 + tx] = tile[tx][k];
}

// ------------------------------------------------------------------------------------------------------------ splat
__global__ __launch_bounds__(256) void lss_cell_interval_kernel(const int32_t *__restrict__ ranks_bev,
                                                                const int32_t *__restrict__ interval_starts,
                                                                const int32_t *__restrict__ counts, int n_int_max,
                                                                int32_t *__restrict__ cell_interval)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_int_max && i < counts[1])
        cell_interval[ranks_bev[interval_starts[i]]] = i;
}

// One wave per chunk of LSS_CHUNK consecutive sorted points, a lane per channel quad (NP passes of 256 channels).  The lanes fetch
// the chunk's indices and compute its probabilities together (one expf per point); the wave then walks the points in order and
// writes one partial row per (chunk, cell) segment: row = chunk + interval index, unique and ascending along the sorted points.
template <int NP>
__global__ __launch_bounds__(256) void lss_splat_chunk_kernel(int C, const float *__restrict__ logits, const float2 *__restrict__ stats,
                                                              const float *__restrict__ feat, const int32_t *__restrict__ ranks_depth,
                                                              const int32_t *__restrict__ ranks_feat, const int32_t *__restrict__ ranks_bev,
                                                              const int32_t *__restrict__ counts, const int32_t *__restrict__ cell_interval,
                                                              float *__restrict__ partial)
{
    const int k = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + threadIdx.x / 64);
    const int ln = threadIdx.x & 63;
    const int n_kept = counts[0];
    const int base = k * LSS_CHUNK;
    if (base >= n_kept)
        return;
    const int n = min(LSS_CHUNK, n_kept - base);
    int my_rf = 0, my_row = 0;
    float my_p = 0.f;
    if (ln < n) {
        my_rf = ranks_feat[base + ln];
        const float2 st = stats[my_rf];
        my_p = expf(logits[ranks_depth[base + ln]] - st.x) * st.y;
        my_row = k + cell_interval[ranks_bev[base + ln]];
    }
    bool mine[NP];
    rac_f4 acc[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        mine[q] = q * 256 + ln * 4 < C;
        acc[q] = rac_f4{0.f, 0.f, 0.f, 0.f};
    }
    int cur = lss_lane_i(my_row, 0);
    auto flush = [&](int row) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            if (mine[q])
                *reinterpret_cast<rac_f4 *>(partial + (size_t)row * C + q * 256 + ln * 4) = acc[q];
            acc[q] = rac_f4{0.f, 0.f, 0.f, 0.f};
        }
    };
    for (int i = 0; i < n; i += 4) {
        rac_f4 f[4][NP];
        int row[4];
        float p[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = min(i + u, n - 1);          // (the tail repeats the last point's loads; its terms are skipped below)
            row[u] = lss_lane_i(my_row, idx);
            p[u] = lss_lane_f(my_p, idx);
            const float *r = feat + (size_t)lss_lane_i(my_rf, idx) * C + ln * 4;
#pragma unroll
            for (int q = 0; q < NP; ++q)
                f[u][q] = mine[q] ? rac_ld4(r + q * 256) : rac_f4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (i + u < n) {
                if (row[u] != cur) {
                    flush(cur);
                    cur = row[u];
                }
#pragma unroll
                for (int q = 0; q < NP; ++q) {
                    acc[q].x = fmaf(f[u][q].x, p[u], acc[q].x);
                    acc[q].y = fmaf(f[u][q].y, p[u], acc[q].y);
                    acc[q].z = fmaf(f[u][q].z, p[u], acc[q].z);
                    acc[q].w = fmaf(f[u][q].w, p[u], acc[q].w);
                }
            }
        }
    }
    flush(cur);
}

// One workgroup per run of LSS_RUN consecutive x cells of one (b, z, y) row: adds each cell's partial rows in chunk order, stages the
// run as [channel][x] in LDS and writes the channel-first output in contiguous x segments.  Empty cells are written as zeros, so the
// output needs no clearing.
__global__ __launch_bounds__(256) void lss_splat_combine_kernel(int C, int X, int Y, int Z, int xruns,
                                                                const int32_t *__restrict__ interval_starts,
                                                                const int32_t *__restrict__ interval_lengths,
                                                                const int32_t *__restrict__ cell_interval,
                                                                const float *__restrict__ partial, float *__restrict__ out)
{
    __shared__ float tile[LSS_MAX_C * (LSS_RUN + 1)];
    const int row = blockIdx.x / xruns, x0 = (blockIdx.x % xruns) * LSS_RUN;
    const int nx = min(LSS_RUN, X - x0);
    const int cell0 = row * X + x0;
    for (int e = threadIdx.x; e < nx * C; e += 256) {
        const int xi = e / C, c = e % C;
        const int iv = cell_interval[cell0 + xi];
        float acc = 0.f;
        if (iv >= 0) {
            const int s = interval_starts[iv], len = interval_lengths[iv];
            const int k0 = s / LSS_CHUNK, k1 = (s + len - 1) / LSS_CHUNK;
            acc = partial[(size_t)(k0 + iv) * C + c];
            for (int k = k0 + 1; k <= k1; ++k)
                acc += partial[(size_t)(k + iv) * C + c];
        }
        tile[c * (LSS_RUN + 1) + xi] = acc;
    }
    __syncthreads();
    const int y = row % Y, z = (row / Y) % Z, b = row / (Y * Z);
    for (int e = threadIdx.x; e < C * LSS_RUN; e += 256) {
        const int c = e / LSS_RUN, xi = e % LSS_RUN;
        if (xi < nx)
            out[((((size_t)b * Z + z) * C + c) * Y + y) * X + x0 + xi] = tile[c * (LSS_RUN + 1) + xi];
    }
}

// ------------------------------------------------------------------------------------------------------------ backward
// One wave per pixel, a lane per channel quad.  The wave walks the pixel's D bins from the cell table; a kept bin gathers the
// cell-major gradient row once and uses it for both the feature gradient (p_d * g) and the bin's score s_d = <g, feat>; a dropped
// bin has s_d = 0 and still gets grad_logit_d = p_d * (0 - sum_d' p_d' s_d') through the softmax.  DCH = ceil(D / 64).
template <int NP, int DCH>
__global__ __launch_bounds__(256) void lss_view_bwd_kernel(int C, int D, int HW, int npix, const float *__restrict__ grad_cell,
                                                           const float *__restrict__ logits, const float2 *__restrict__ stats,
                                                           const float *__restrict__ feat, const int32_t *__restrict__ cells,
                                                           float *__restrict__ grad_feat, float *__restrict__ grad_logits)
{
    const int pix = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + threadIdx.x / 64);
    const int ln = threadIdx.x & 63;
    if (pix >= npix)
        return;
    const size_t col = (size_t)(pix / HW) * D * HW + pix % HW;       // bin d of this pixel sits at col + d * HW
    const float2 st = stats[pix];
    bool mine[NP];
    rac_f4 f[NP], acc[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        mine[q] = q * 256 + ln * 4 < C;
        f[q] = mine[q] ? rac_ld4(feat + (size_t)pix * C + q * 256 + ln * 4) : rac_f4{0.f, 0.f, 0.f, 0.f};
        acc[q] = rac_f4{0.f, 0.f, 0.f, 0.f};
    }
    float my_p[DCH], my_s[DCH];
    float S = 0.f;
#pragma unroll
    for (int ch = 0; ch < DCH; ++ch) {
        const int d = ch * 64 + ln;
        int c = -1;
        float p = 0.f;
        if (d < D) {
            c = cells[col + (size_t)d * HW];
            p = expf(logits[col + (size_t)d * HW] - st.x) * st.y;
        }
        float sv = 0.f;
        const int n = min(64, D - ch * 64);
        for (int i = 0; i < n; ++i) {
            const int ci = lss_lane_i(c, i);
            if (ci < 0)
                continue;
            const float pi = lss_lane_f(p, i);
            float dot = 0.f;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const rac_f4 g = mine[q] ? rac_ld4(grad_cell + (size_t)ci * C + q * 256 + ln * 4) : rac_f4{0.f, 0.f, 0.f, 0.f};
                dot += (g.x * f[q].x + g.y * f[q].y) + (g.z * f[q].z + g.w * f[q].w);
                acc[q].x = fmaf(g.x, pi, acc[q].x);
                acc[q].y = fmaf(g.y, pi, acc[q].y);
                acc[q].z = fmaf(g.z, pi, acc[q].z);
                acc[q].w = fmaf(g.w, pi, acc[q].w);
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1)
                dot += __shfl_xor(dot, off, 64);
            S = fmaf(pi, dot, S);
            if (ln == i)
                sv = dot;
        }
        my_p[ch] = p;
        my_s[ch] = sv;
    }
#pragma unroll
    for (int q = 0; q < NP; ++q)
        if (mine[q])
            *reinterpret_cast<rac_f4 *>(grad_feat + (size_t)pix * C + q * 256 + ln * 4) = acc[q];
#pragma unroll
    for (int ch = 0; ch < DCH; ++ch) {
        const int d = ch * 64 + ln;
        if (d < D)
            grad_logits[col + (size_t)d * HW] = my_p[ch] * (my_s[ch] - S);
    }
}

// ------------------------------------------------------------------------------------------------------------ entry points
static bool lss_c_ok(int c) { return c >= 4 && c <= LSS_MAX_C && c % 4 == 0; }

extern "C" int rac_lss_cells_fwd(const float *img2lidar, const float *depth_tab, const float *v_tab, const float *u_tab, int32_t *cells,
                                 int BN, int N, int D, int H, int W, float lower_x, float lower_y, float lower_z, float interval_x,
                                 float interval_y, float interval_z, int X, int Y, int Z, void *stream)
{
    RAC_CHECK_ARG(BN >= 1 && N >= 1 && BN % N == 0 && D >= 1 && H >= 1 && W >= 1 && X >= 1 && Y >= 1 && Z >= 1,
                  "rac_lss_cells_fwd: BN=%d N=%d D=%d H=%d W=%d grid=%dx%dx%d", BN, N, D, H, W, X, Y, Z);
    RAC_CHECK_ARG(D <= 65535 && BN <= 65535 && (long)BN * D * H * W < (1L << 31) && (long)(BN / N) * X * Y * Z < (1L << 31),
                  "rac_lss_cells_fwd: sizes exceed the int32 tables");
    RAC_CHECK_ARG(interval_x > 0.f && interval_y > 0.f && interval_z > 0.f, "rac_lss_cells_fwd: non-positive cell size");
    RAC_CHECK_ARG(img2lidar && depth_tab && v_tab && u_tab && cells, "rac_lss_cells_fwd: null pointer");
    hipLaunchKernelGGL(lss_cells_kernel, dim3((H * W + 255) / 256, D, BN), dim3(256), 0, (hipStream_t)stream, img2lidar, depth_tab,
                       v_tab, u_tab, cells, N, D, H, W, lower_x, lower_y, lower_z, interval_x, interval_y, interval_z, X, Y, Z);
    return rac_launch_status("rac_lss_cells_fwd");
}

extern "C" int rac_lss_tables_fwd(const int32_t *cells, int32_t *ranks_bev, int32_t *ranks_depth, int32_t *ranks_feat,
                                  int32_t *interval_starts, int32_t *interval_lengths, int32_t *counts, int32_t *workspace,
                                  int n_points, int n_cells, int D, int HW, void *stream)
{
    RAC_CHECK_ARG(n_points >= 1 && n_cells >= 1 && n_cells < (1 << 30) && D >= 1 && HW >= 1 && n_points % (D * HW) == 0,
                  "rac_lss_tables_fwd: n_points=%d n_cells=%d D=%d HW=%d", n_points, n_cells, D, HW);
    RAC_CHECK_ARG(cells && ranks_bev && ranks_depth && ranks_feat && interval_starts && interval_lengths && counts && workspace,
                  "rac_lss_tables_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    int32_t *count = workspace, *cursor = workspace + n_cells, *cell_start = workspace + 2 * (size_t)n_cells,
            *slots = workspace + 3 * (size_t)n_cells;
    const int n_int_max = n_cells < n_points ? n_cells : n_points;
    const unsigned pblocks = (unsigned)((n_points + 255) / 256);
    hipLaunchKernelGGL(lss_fill_i32_kernel, dim3((unsigned)((2 * (long)n_cells + 255) / 256)), dim3(256), 0, st, workspace, 2 * n_cells,
                       0);
    hipLaunchKernelGGL(lss_hist_kernel, dim3(pblocks), dim3(256), 0, st, cells, n_points, count);
    hipLaunchKernelGGL(lss_scan_kernel, dim3(1), dim3(1024), 0, st, count, n_cells, n_int_max, cell_start, interval_starts,
                       interval_lengths, counts);
    hipLaunchKernelGGL(lss_fill_kernel, dim3(pblocks), dim3(256), 0, st, cells, n_points, cell_start, cursor, slots);
    hipLaunchKernelGGL(lss_order_kernel, dim3(pblocks), dim3(256), 0, st, cells, slots, cell_start, count, counts, n_points, D, HW,
                       ranks_bev, ranks_depth, ranks_feat);
    return rac_launch_status("rac_lss_tables_fwd");
}

extern "C" int rac_lss_softmax_stats_fwd(const float *logits, float *stats, int BN, int D, int HW, void *stream)
{
    RAC_CHECK_ARG(BN >= 1 && D >= 1 && HW >= 1 && (long)BN * D * HW < (1L << 31), "rac_lss_softmax_stats_fwd: BN=%d D=%d HW=%d", BN, D,
                  HW);
    RAC_CHECK_ARG(logits && stats, "rac_lss_softmax_stats_fwd: null pointer");
    const int npix = BN * HW;
    hipLaunchKernelGGL(lss_softmax_stats_kernel, dim3((npix + 63) / 64), dim3(64), 0, (hipStream_t)stream, logits,
                       reinterpret_cast<float2 *>(stats), npix, D, HW);
    return rac_launch_status("rac_lss_softmax_stats_fwd");
}

extern "C" int rac_lss_transpose_fwd(const float *src, float *dst, int batch, int rows, int cols, void *stream)
{
    RAC_CHECK_ARG(batch >= 1 && batch <= 65535 && rows >= 1 && cols >= 1 && (rows + 31) / 32 <= 65535,
                  "rac_lss_transpose_fwd: batch=%d rows=%d cols=%d", batch, rows, cols);
    RAC_CHECK_ARG(src && dst, "rac_lss_transpose_fwd: null pointer");
    hipLaunchKernelGGL(lss_transpose_kernel, dim3((cols + 31) / 32, (rows + 31) / 32, batch), dim3(256), 0, (hipStream_t)stream, src,
                       dst, rows, cols);
    return rac_launch_status("rac_lss_transpose_fwd");
}

extern "C" int rac_lss_splat_fwd(const float *logits, const float *stats, const float *feat, const int32_t *ranks_depth,
                                 const int32_t *ranks_feat, const int32_t *ranks_bev, const int32_t *interval_starts,
                                 const int32_t *interval_lengths, const int32_t *counts, int32_t *cell_interval, float *partial,
                                 float *out, int n_points, int B, int C, int X, int Y, int Z, void *stream)
{
    RAC_CHECK_ARG(lss_c_ok(C), "rac_lss_splat_fwd: C=%d (multiples of 4 up to %d)", C, LSS_MAX_C);
    RAC_CHECK_ARG(n_points >= 1 && B >= 1 && X >= 1 && Y >= 1 && Z >= 1 && (long)B * X * Y * Z < (1L << 31),
                  "rac_lss_splat_fwd: n_points=%d B=%d grid=%dx%dx%d", n_points, B, X, Y, Z);
    RAC_CHECK_ARG(logits && stats && feat && ranks_depth && ranks_feat && ranks_bev && interval_starts && interval_lengths && counts &&
                      cell_interval && partial && out,
                  "rac_lss_splat_fwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int n_cells = B * Z * Y * X;
    const int n_int_max = n_cells < n_points ? n_cells : n_points;
    const int n_chunks = (n_points + LSS_CHUNK - 1) / LSS_CHUNK;
    const int xruns = (X + LSS_RUN - 1) / LSS_RUN;
    hipLaunchKernelGGL(lss_fill_i32_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, st, cell_interval, n_cells,
                       -1);                                                                         // -1: empty cell
    hipLaunchKernelGGL(lss_cell_interval_kernel, dim3((n_int_max + 255) / 256), dim3(256), 0, st, ranks_bev, interval_starts, counts,
                       n_int_max, cell_interval);
    const float2 *st2 = reinterpret_cast<const float2 *>(stats);
    if (C <= 256)
        hipLaunchKernelGGL(lss_splat_chunk_kernel<1>, dim3((n_chunks + 3) / 4), dim3(256), 0, st, C, logits, st2, feat, ranks_depth,
                           ranks_feat, ranks_bev, counts, cell_interval, partial);
    else
        hipLaunchKernelGGL(lss_splat_chunk_kernel<2>, dim3((n_chunks + 3) / 4), dim3(256), 0, st, C, logits, st2, feat, ranks_depth,
                           ranks_feat, ranks_bev, counts, cell_interval, partial);
    hipLaunchKernelGGL(lss_splat_combine_kernel, dim3((unsigned)(B * Z * Y * xruns)), dim3(256), 0, st, C, X, Y, Z, xruns,
                       interval_starts, interval_lengths, cell_interval, partial, out);
    return rac_launch_status("rac_lss_splat_fwd");
}

extern "C" int rac_lss_view_bwd(const float *grad_cell, const float *logits, const float *stats, const float *feat,
                                const int32_t *cells, float *grad_feat, float *grad_logits, int BN, int C, int D, int HW, void *stream)
{
    RAC_CHECK_ARG(lss_c_ok(C), "rac_lss_view_bwd: C=%d (multiples of 4 up to %d)", C, LSS_MAX_C);
    RAC_CHECK_ARG(BN >= 1 && D >= 1 && D <= LSS_MAX_D && HW >= 1 && (long)BN * D * HW < (1L << 31),
                  "rac_lss_view_bwd: BN=%d D=%d (at most %d) HW=%d", BN, D, LSS_MAX_D, HW);
    RAC_CHECK_ARG(grad_cell && logits && stats && feat && cells && grad_feat && grad_logits, "rac_lss_view_bwd: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const int npix = BN * HW;
    const float2 *st2 = reinterpret_cast<const float2 *>(stats);
    const int dch = (D + 63) / 64;
#define LSS_BWD(NP_, DCH_)                                                                                                            \
    hipLaunchKernelGGL((lss_view_bwd_kernel<NP_, DCH_>), dim3((npix + 3) / 4), dim3(256), 0, st, C, D, HW, npix, grad_cell, logits, st2, \
                       feat, cells, grad_feat, grad_logits)
    if (C <= 256) {
        if (dch == 1) LSS_BWD(1, 1);
        else if (dch == 2) LSS_BWD(1, 2);
        else LSS_BWD(1, 4);
    } else {
        if (dch == 1) LSS_BWD(2, 1);
        else if (dch == 2) LSS_BWD(2, 2);
        else LSS_BWD(2, 4);
    }
#undef LSS_BWD
    return rac_launch_status("rac_lss_view_bwd");
}
