// bev_fused_bwd.hip -- backward of rac_bev_sampling_fwd (bev_fused.hip) as ONE kernel (gfx950), float32 values.  One kernel source,
// bev_sampling_bwd_d64_kernel<ONE>, in two instantiations: rac_bev_sampling_bwd launches the one with B fixed at 1 at compile time (its
// r % B, r / B and b * ... fold away), rac_bev_sampling_bwd_batch the one with B read from the arguments, for every B >= 1.
//
// Forward, per (q, h) and channel c:   out[c] = sum_t qw[t] * sum_p aw[h,p] * bilinear(V[t], loc[t,h,p])[h,c]
// with qw = softmax_T(queue logits), aw = softmax_P(scale logits of head h) and loc the keypoint chain
//   base[h,p] = centre + R(yaw) (exp(w,l) * offset[h,p])                      (T-invariant; box table of rac_box_prep_fwd)
//   loc[t,h,p] = clamp01(polar_jitter(warp(base - vel * time_diff[t]), doff[p % D]))
//   doff[d] = depth_base[d] + (2 sigmoid(ray[d]) - 1) * d_region / D / 2.
// Nothing of the forward is saved: keypoints and softmaxes are recomputed with the forward's own device functions
// (bev_device.h), so the locations are the forward's bits; the bilinear footprint is the gathers' shared rac_footprint.
//
// For B > 1 the reference pairs row r = 0 .. B*T-1 of the value frames (b-major: frame and output slot (b_o, t_o) = (r / T, r % T),
// whose frame weight softmax_T(queue[b_o, q])[t_o] and gradient row grad_out[b_o, q] it takes) with the keypoints and point weights
// of (b_l, t_l) = (r % B, r / B) (bev_fused.hip, quirk Q2).  out[b_o, q] then depends on the logits of query q in several samples,
// and the gradients of (b_l, q) collect terms from several output rows.
//
// Workgroup = query index q of ALL B samples (all heads), 256 threads, so every sum over heads, frames, points and output rows has
// one writer and a fixed order.  Phases over the B*T rows, the per-sample pieces indexed by b_l, the frame weights and grad_out rows
// by b_o:
//   phase A  T-invariant pieces into LDS (base points, depth offsets, both softmaxes, the grad_out rows);
//   phase B  one thread per keypoint (r, h, p): location and combined weight aw * qw into LDS; the keypoints are the forward's:
//            bev_warp from the LDS base points at B == 1, bev_keypoint_from_query at B > 1;
//   phase C  the gather half, as rac_msda_bwd: a 16-lane group per keypoint, lane c owns channels c + 16 j; value taps loaded,
//            grad_value scattered with float atomics (whole 64-byte segments), the three channel sums (d/d weight, d/d x,
//            d/d y) by a butterfly inside the group; lane 0 keeps them in LDS (and writes the optional debug outputs);
//   phase D  the chain tail, one thread per keypoint: clamp, polar jitter and warp backwards -> d/d base point, d/d doff;
//   phase E  fixed-order sums: over frames -> offsets and box table; softmax backwards over P and over T; ray logits.
// Everything except grad_value is written once, from sums in a fixed order (bit-reproducible, and the same bits from both
// instantiations at B == 1).  Velocity and time_diff get no gradient (the reference detaches the velocity).
#include "bev_device.h"
#include "gather_device.h"

struct BevBwdArgs {
    const float *value;      // [B*T, H*W, heads, 64]
    const float *box;        // [B,Q,8]
    const float *qbox;       // [B,Q,10]
    const float *off, *ray, *scale, *queue;   // rows (b * Q + q) of the Linear outputs (ld_*)
    const float *time_diff;  // [B,T]
    const float *grad_out;   // [B,Q,heads*64]
    float *gvalue;           // [B*T, H*W, heads, 64], zero-filled by the caller
    float *goff, *gray, *gscale, *gqueue;     // rows (gld_*)
    float *gbox;             // [B,Q,8]
    float *gloc_out, *gattn_out;              // optional [B,Q,heads,T,P,2] / [B,Q,heads,T,P], indexed by the output slot (b_o, t_o)
    float depth_base[BEV_MAX_DEPTH];
    float pc[6];
    float d_region;
    int B, T, Q, heads, NP, D, P, H, W;
    int ld_off, ld_ray, ld_scale, ld_queue;
    int gld_off, gld_ray, gld_scale, gld_queue;
};

#define BEV_BWD_BOX_LD 16    /* LDS floats per sample for the box table row [8] and the velocity [2] */

// LDS floats: per keypoint 6 (loc x, loc y -> d/d doff; weight; d/d weight; d/d x -> d/d base x; d/d y -> d/d base y), per (b, h, p) 8,
// per (b, head) 64, per row 3, per sample the depth and box vectors
static size_t bev_bwd_lds_floats(int B, int heads, int T, int P)
{
    return (size_t)B * ((size_t)heads * T * P * 6 + (size_t)heads * P * 8 + (size_t)heads * 64 + (size_t)T * 3 + BEV_MAX_DEPTH * 2 + BEV_BWD_BOX_LD);
}

// Backward of bev_warp + bev_polar_jitter at one keypoint.  (px, py): base point, (gx, gy): gradient with respect to the clamped
// location.  Returns the gradient with respect to the base point (gb2) and to the distance offset.  The clamp passes the
// gradient where 0 <= u <= 1 (torch.clamp); a non-finite u passes none.
__device__ __forceinline__ float bev_warp_bwd(const float *pc, float px, float py, float vx, float vy, float td, float doff,
                                              float gx, float gy, float *gb2)
{
    const float sx = pc[3] - pc[0], sy = pc[4] - pc[1];
    px -= vx * td;
    py -= vy * td;
    const float nx = (px - pc[0]) / sx, ny = (py - pc[1]) / sy;
    const float ex = nx * 102.4f - 51.2f, ey = ny * 102.4f - 51.2f;
    const float r2 = ex * ex + ey * ey, r = sqrtf(r2);
    const float dist = r / 65.0f + doff;
    const float th = fmodf(atan2f(ey, ex) + BEV_TWO_PI, BEV_TWO_PI) / BEV_TWO_PI;
    const float ang = th * BEV_TWO_PI, rad = dist * 65.0f;
    const float cs = cosf(ang), sn = sinf(ang);
    const float ux = (51.2f + rad * cs) / 102.4f, uy = (51.2f + rad * sn) / 102.4f;
    const float gux = (ux >= 0.f && ux <= 1.f) ? gx / 102.4f : 0.f;
    const float guy = (uy >= 0.f && uy <= 1.f) ? gy / 102.4f : 0.f;
    const float g_rad = gux * cs + guy * sn;               // = d/d r (dist = r / 65 + doff, rad = 65 dist)
    const float g_ang = rad * (guy * cs - gux * sn);       // = d/d atan2 (the fmod and the two 2 pi factors have slope 1)
    // r = 0 (a keypoint on the map centre): sqrt and atan2 have no derivative there; no gradient to the base point
    const float ir = r2 > 0.f ? 1.f / r : 0.f, ir2 = r2 > 0.f ? 1.f / r2 : 0.f;
    const float g_ex = g_rad * ex * ir - g_ang * ey * ir2;
    const float g_ey = g_rad * ey * ir + g_ang * ex * ir2;
    gb2[0] = g_ex * 102.4f / sx;
    gb2[1] = g_ey * 102.4f / sy;
    return g_rad * 65.0f;
}

// The footprint of a keypoint, its pixel coordinates y * H - 0.5, x * W - 0.5 rounded operation by operation (no fused multiply-add) as
// rac_footprint rounds its differences and as the float64 references form them: on a map whose size is not a power of two a
// contracted fma(y, H, -0.5) differs by an ulp of the coordinate, which a tap weight close to 0 shows as 1e-5 of its value.
__device__ __forceinline__ RacFootprint bev_bwd_footprint(float x, float y, int H, int W)
{
#pragma clang fp contract(off)
    const float h_im = y * (float)H - 0.5f, w_im = x * (float)W - 0.5f;
    return rac_footprint(h_im, w_im, H, W);
}

// ONE: B is 1 at compile time (rac_bev_sampling_bwd); otherwise a.B (rac_bev_sampling_bwd_batch, any B >= 1)
template <bool ONE>
__global__ __launch_bounds__(256) void bev_sampling_bwd_d64_kernel(const BevBwdArgs a)
{
    extern __shared__ float smem[];
    const int tid = threadIdx.x, q = blockIdx.x;
    const int B = ONE ? 1 : a.B, T = a.T, P = a.P, D = a.D, Hn = a.heads, HP = Hn * P, R = B * T, N = R * HP, BHP = B * HP;
    const int H = a.H, W = a.W;
    // the sample b of item i = b * n + e of B * n items: 0 where B is fixed at 1, which spares the division the compiler cannot drop
    // (it does not see i < n)
    const auto sample = [](int i, int n) { return ONE ? 0 : i / n; };
    // keypoint index k = (r * heads + h) * P + p: value-frame-major
    float *kx = smem;              // [N] loc x                 -> phase D: d/d doff
    float *ky = kx + N;            // [N] loc y
    float *kw = ky + N;            // [N] aw[b_l,h,p] * qw[b_o,t_o]
    float *ks = kw + N;            // [N] sum_c g[c] * bilinear[c]
    float *kgx = ks + N;           // [N] d/d loc x (weight included) -> phase D: d/d base x
    float *kgy = kgx + N;          // [N] d/d loc y                   -> phase D: d/d base y
    float *sbase = kgy + N;        // [B][HP][2]
    float *soff = sbase + BHP * 2; // [B][HP][2] the offsets as read
    float *saw = soff + BHP * 2;   // [B][HP]
    float *sgb = saw + BHP;        // [B][HP][2] sum over frames of d/d base point
    float *sdaw = sgb + BHP * 2;   // [B][HP] d/d aw
    float *sg = sdaw + BHP;        // [B][heads][64] grad_out rows
    float *sqw = sg + B * Hn * 64; // [R] frame weights, by output slot r = b_o * T + t_o
    float *sdqw = sqw + R;         // [R] d/d qw
    float *std_ = sdqw + R;        // [B][T] time_diff
    float *sdoff = std_ + R;       // [B][BEV_MAX_DEPTH]
    float *ssig = sdoff + B * BEV_MAX_DEPTH;   // [B][BEV_MAX_DEPTH] sigmoid(ray)
    float *sbox = ssig + B * BEV_MAX_DEPTH;    // [B][BEV_BWD_BOX_LD]: box table row [0..7], velocity [8..9]

    // phase A
    for (int i = tid; i < B * 10; i += 256) {
        const int b = sample(i, 10), e = i - b * 10;
        const size_t row = (size_t)b * a.Q + q;
        sbox[b * BEV_BWD_BOX_LD + e] = e < 8 ? a.box[row * 8 + e] : a.qbox[row * 10 + e];
    }
    for (int i = tid; i < B * Hn * 64; i += 256) {
        const int b = sample(i, Hn * 64), e = i - b * (Hn * 64);
        sg[i] = a.grad_out[((size_t)b * a.Q + q) * Hn * 64 + e];
    }
    for (int i = tid; i < R; i += 256)
        std_[i] = a.time_diff[i];
    for (int i = tid; i < BHP; i += 256) {
        const int b = sample(i, HP), hp = i - b * HP;
        const size_t row = (size_t)b * a.Q + q;
        const float *bt = a.box + row * 8;
        const float *o = a.off + row * a.ld_off + (size_t)hp * 2;
        const float btr[8] = {bt[0], bt[1], 0.f, bt[3], bt[4], 0.f, bt[6], bt[7]};
        const float o0 = o[0], o1 = o[1];
        soff[i * 2] = o0;
        soff[i * 2 + 1] = o1;
        bev_base_point(btr, o0, o1, sbase + i * 2);
    }
    for (int i = (tid + 128) & 255; i < B * D; i += 256) {
        const int b = sample(i, D), dd = i - b * D;
        const float sgm = bev_sigmoid(a.ray[((size_t)b * a.Q + q) * a.ld_ray + dd]);
        ssig[b * BEV_MAX_DEPTH + dd] = sgm;
        sdoff[b * BEV_MAX_DEPTH + dd] = bev_depth_offset(sgm, a.depth_base[dd], a.d_region, D);
    }
    {
        // the softmaxes across the lanes of a wave, as the forward forms them: items 0 .. B*heads-1 are the point weights of
        // (b, h), items B*heads .. B*heads+B-1 the frame weights of b; wave w takes items w, w + 4, ... (wave-uniform)
        const int wv = tid >> 6, ln = tid & 63;
        for (int it = wv; it < B * Hn + B; it += 4) {
            if (it < B * Hn) {
                const int b = sample(it, Hn), h = it - b * Hn;
                const float lg = ln < P ? a.scale[((size_t)b * a.Q + q) * a.ld_scale + (size_t)h * P + ln] : -INFINITY;
                const float w = bev_wave_softmax(lg, ln < P);
                if (ln < P)
                    saw[it * P + ln] = w;
            } else {
                const int b = it - B * Hn;
                const float lg = ln < T ? a.queue[((size_t)b * a.Q + q) * a.ld_queue + ln] : -INFINITY;
                const float w = bev_wave_softmax(lg, ln < T);
                if (ln < T)
                    sqw[b * T + ln] = w;
            }
        }
    }
    __syncthreads();
    // phase B: per-row keypoints, those of the paired sample (b_l, t_l)
    for (int k = tid; k < N; k += 256) {
        const int r = k / HP, hp = k - r * HP, p = hp % P;
        const int bl = r % B, tl = r / B;
        const float *bx = sbox + bl * BEV_BWD_BOX_LD;
        float loc[2];
        if (B == 1) {
            bev_warp(a.pc, sbase[hp * 2], sbase[hp * 2 + 1], bx[8], bx[9], std_[r], sdoff[p % D], loc);
        } else {
            const size_t row = (size_t)bl * a.Q + q;
            bev_keypoint_from_query(a.pc, a.qbox + row * 10, a.off + row * a.ld_off + (size_t)hp * 2, a.ray[row * a.ld_ray + p % D],
                                    std_[bl * T + tl], a.depth_base[p % D], a.d_region, D, loc);
        }
        kx[k] = loc[0];
        ky[k] = loc[1];
        kw[k] = saw[bl * HP + hp] * sqw[r];
    }
    __syncthreads();
    // phase C: gather half.  16 groups of 16 lanes; group g takes keypoints g, g + 16, ...
    {
        const int lane16 = tid & 15, grp = tid >> 4;
        const int stride = Hn * 64;
        for (int k = grp; k < N; k += 16) {
            const int r = k / HP, hp = k - r * HP, h = hp / P, p = hp - h * P;
            const int bo = sample(r, T), to = r - bo * T;
            const float x = kx[k], y = ky[k], at = kw[k];
            float g[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                g[j] = sg[(bo * Hn + h) * 64 + 16 * j + lane16];
            const RacFootprint f = bev_bwd_footprint(x, y, H, W);
            const int h_low = f.h_low, w_low = f.w_low, h_high = h_low + 1, w_high = w_low + 1;
            const float lh = f.lh, lw = f.lw, hh = f.hh, hw = f.hw;
            const size_t map = ((size_t)r * H * W * Hn + h) * 64 + lane16;
            const float *base = a.value + map;
            float *gbase = a.gvalue + map;
            const size_t o[4] = {((size_t)h_low * W + w_low) * stride, ((size_t)h_low * W + w_high) * stride,
                                 ((size_t)h_high * W + w_low) * stride, ((size_t)h_high * W + w_high) * stride};
            const float tw[4] = {hh * hw, hh * lw, lh * hw, lh * lw};
            const float dh[4] = {-hw, -lw, hw, lw}, dw[4] = {-hh, hh, -lh, lh};
            float v[4][4];
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    v[c][j] = f.ok[c] ? base[o[c] + 16 * j] : 0.f;
            float sv = 0.f, sh = 0.f, sw_ = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (f.ok[c]) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        atomicAdd(gbase + o[c] + 16 * j, tw[c] * (g[j] * at));
                }
                const float dot = (v[c][0] * g[0] + v[c][1] * g[1]) + (v[c][2] * g[2] + v[c][3] * g[3]);
                sv += tw[c] * dot;
                sh += dh[c] * dot;
                sw_ += dw[c] * dot;
            }
            sv = rac_group_sum16(sv);
            sh = rac_group_sum16(sh);
            sw_ = rac_group_sum16(sw_);
            if (lane16 == 0) {
                const float gx = (float)W * sw_ * at, gy = (float)H * sh * at;
                ks[k] = sv;
                kgx[k] = gx;
                kgy[k] = gy;
                const size_t e = ((((size_t)bo * a.Q + q) * Hn + h) * T + to) * P + p;
                if (a.gattn_out)
                    a.gattn_out[e] = sv;
                if (a.gloc_out) {
                    a.gloc_out[e * 2] = gx;
                    a.gloc_out[e * 2 + 1] = gy;
                }
            }
        }
    }
    __syncthreads();
    // phase D: chain tail per keypoint, through the chain of (b_l, t_l)
    for (int k = tid; k < N; k += 256) {
        const int r = k / HP, hp = k - r * HP, p = hp % P;
        const int bl = r % B, tl = r / B;
        const float *bx = sbox + bl * BEV_BWD_BOX_LD, *bp = sbase + (bl * HP + hp) * 2;
        float gb[2];
        const float gd = bev_warp_bwd(a.pc, bp[0], bp[1], bx[8], bx[9], std_[bl * T + tl], sdoff[bl * BEV_MAX_DEPTH + p % D], kgx[k], kgy[k], gb);
        kgx[k] = gb[0];
        kgy[k] = gb[1];
        kx[k] = gd;
    }
    __syncthreads();
    // phase E1: sums over the T rows of each sample b_l (r = t_l * B + b_l, t_l ascending) per (h, p); d/d qw per row; d/d doff per
    // depth slot.  Fixed order.
    for (int i = tid; i < BHP; i += 256) {
        const int b = sample(i, HP), hp = i - b * HP;
        const float *bx = sbox + b * BEV_BWD_BOX_LD;
        float gbx = 0.f, gby = 0.f, daw = 0.f;
        for (int t = 0; t < T; ++t) {
            const int r = t * B + b;
            gbx += kgx[r * HP + hp];
            gby += kgy[r * HP + hp];
            daw += sqw[r] * ks[r * HP + hp];
        }
        sgb[i * 2] = gbx;
        sgb[i * 2 + 1] = gby;
        sdaw[i] = daw;
        float *go = a.goff + ((size_t)b * a.Q + q) * a.gld_off + (size_t)hp * 2;
        go[0] = bx[3] * (gbx * bx[6] + gby * bx[7]);
        go[1] = bx[4] * (gby * bx[6] - gbx * bx[7]);
    }
    for (int r = 255 - tid; r < R; r += 256) {
        const float *aw = saw + (r % B) * HP;
        float dq = 0.f;
        for (int i = 0; i < HP; ++i)
            dq += aw[i] * ks[r * HP + i];
        sdqw[r] = dq;
    }
    for (int i = (tid + 128) & 255; i < B * D; i += 256) {
        const int b = sample(i, D), dd = i - b * D;
        float gd = 0.f;
        for (int t = 0; t < T; ++t)
            for (int h = 0; h < Hn; ++h)
                for (int p = dd; p < P; p += D)
                    gd += kx[((t * B + b) * Hn + h) * P + p];
        const float sgm = ssig[b * BEV_MAX_DEPTH + dd];
        a.gray[((size_t)b * a.Q + q) * a.gld_ray + dd] = gd * (sgm * (1.f - sgm)) * 2.f * a.d_region / (float)D / 2.f;
    }
    __syncthreads();
    // phase E2: softmax backwards, box table
    for (int i = tid; i < BHP; i += 256) {
        const int b = sample(i, HP), hp = i - b * HP, h = hp / P;
        const float *aw = saw + (b * Hn + h) * P, *da = sdaw + (b * Hn + h) * P;
        float dot = 0.f;
        for (int p = 0; p < P; ++p)
            dot += aw[p] * da[p];
        a.gscale[((size_t)b * a.Q + q) * a.gld_scale + hp] = saw[i] * (sdaw[i] - dot);
    }
    for (int r = 255 - tid; r < R; r += 256) {
        const int bo = sample(r, T), to = r - bo * T;
        float dot = 0.f;
        for (int u = 0; u < T; ++u)
            dot += sqw[bo * T + u] * sdqw[bo * T + u];
        a.gqueue[((size_t)bo * a.Q + q) * a.gld_queue + to] = sqw[r] * (sdqw[r] - dot);
    }
    for (int i = (tid + 192) & 255; i < B * 8; i += 256) {
        const int b = sample(i, 8), e = i & 7;
        const float *bx = sbox + b * BEV_BWD_BOX_LD;
        const float bw = bx[3], bl = bx[4], bcs = bx[6], bsn = bx[7];
        float s = 0.f;
        for (int j = 0; j < HP; ++j) {
            const float gbx = sgb[(b * HP + j) * 2], gby = sgb[(b * HP + j) * 2 + 1];
            const float o0 = soff[(b * HP + j) * 2], o1 = soff[(b * HP + j) * 2 + 1];
            const float dx = bw * o0, dy = bl * o1;
            float term = 0.f;
            if (e == 0) term = gbx;
            else if (e == 1) term = gby;
            else if (e == 3) term = o0 * (gbx * bcs + gby * bsn);
            else if (e == 4) term = o1 * (gby * bcs - gbx * bsn);
            else if (e == 6) term = gbx * dx + gby * dy;
            else if (e == 7) term = gby * dx - gbx * dy;
            s += term;
        }
        a.gbox[((size_t)b * a.Q + q) * 8 + e] = s;     // (entries 2 and 5, height and its centre, are not read by the forward: 0)
    }
}

#define BEV_BWD_LDS_LIMIT (160 * 1024)    /* the LDS of one CU (MI355X): what a single workgroup may take */

// the argument checks and the launch of rac_bev_sampling_bwd (batch = false: B <= 1, the LDS a launch may ask for by default) and
// rac_bev_sampling_bwd_batch (any B >= 1, up to the LDS of a CU)
static int bev_bwd_launch(const char *fn, bool batch, const void *value, const float *query_bbox, const float *box_table, const float *offsets,
                          const float *ray_logits, const float *scale_logits, const float *queue_logits,
                          const float *time_diff, const float *grad_out, float *grad_value, float *grad_offsets,
                          float *grad_ray, float *grad_scale, float *grad_queue, float *grad_box, float *grad_loc_out,
                          float *grad_attn_out, int ld_off, int ld_ray, int ld_scale, int ld_queue, int gld_off,
                          int gld_ray, int gld_scale, int gld_queue, int B, int T, int Q, int heads, int NP, int D, int H,
                          int W, int dim, const float *pc_range, const float *depth_base, float d_region, int dtype,
                          void *stream)
{
    RAC_CHECK_ARG(dim == 64, "%s: dim=%d (the fused kernel is built for 64 channels per head)", fn, dim);
    RAC_CHECK_ARG(B >= (batch ? 1 : 0) && Q >= 0 && T >= 1 && heads >= 1 && NP >= 1 && D >= 1 && D <= BEV_MAX_DEPTH && H >= 1 && W >= 1,
                  "%s: bad sizes B=%d T=%d Q=%d heads=%d NP=%d D=%d H=%d W=%d", fn, B, T, Q, heads, NP, D, H, W);
    RAC_CHECK_ARG(dtype == RAC_F32, "%s: dtype %d (float32 value streams only; bf16 / int16 streams take the unfused route)", fn, dtype);
    RAC_CHECK_ARG(batch || B <= 1, "%s: B=%d (B == 1 only: a batch takes the unfused route, which pairs frames and batches as the reference does)", fn, B);
    const int P = NP * D;
    RAC_CHECK_ARG(T <= 64 && P <= 64, "%s: T=%d frames or NP*D=%d points (max 64 each: one lane per term in the softmaxes)", fn, T, P);
    RAC_CHECK_ARG(ld_off >= heads * P * 2 && ld_ray >= D && ld_scale >= heads * P && ld_queue >= T,
                  "%s: row strides ld_off=%d ld_ray=%d ld_scale=%d ld_queue=%d narrower than their rows", fn, ld_off, ld_ray, ld_scale, ld_queue);
    RAC_CHECK_ARG(gld_off >= heads * P * 2 && gld_ray >= D && gld_scale >= heads * P && gld_queue >= T,
                  "%s: gradient row strides gld_off=%d gld_ray=%d gld_scale=%d gld_queue=%d narrower than their rows", fn, gld_off, gld_ray,
                  gld_scale, gld_queue);
    const size_t lds = bev_bwd_lds_floats(batch ? B : 1, heads, T, P) * sizeof(float);      // (batch = false checks one sample's at B = 0 too)
    if (batch)
        RAC_CHECK_ARG(lds <= BEV_BWD_LDS_LIMIT,
                      "%s: B=%d samples of heads*T*NP*D=%d keypoints need %zu bytes of LDS staging (one workgroup covers a query index of all samples; limit %d)",
                      fn, B, heads * T * P, lds, BEV_BWD_LDS_LIMIT);
    else
        RAC_CHECK_ARG(lds <= 64 * 1024, "%s: heads*T*NP*D=%d keypoints per query too many for the LDS staging", fn, heads * T * P);
    if (B == 0 || Q == 0)
        return 0;
    RAC_CHECK_ARG(value && query_bbox && box_table && offsets && ray_logits && scale_logits && queue_logits && time_diff && grad_out &&
                      grad_value && grad_offsets && grad_ray && grad_scale && grad_queue && grad_box && pc_range && depth_base,
                  "%s: null pointer", fn);
    BevBwdArgs a;
    a.value = (const float *)value; a.box = box_table; a.qbox = query_bbox;
    a.off = offsets; a.ray = ray_logits; a.scale = scale_logits; a.queue = queue_logits;
    a.time_diff = time_diff; a.grad_out = grad_out;
    a.gvalue = grad_value; a.goff = grad_offsets; a.gray = grad_ray; a.gscale = grad_scale; a.gqueue = grad_queue; a.gbox = grad_box;
    a.gloc_out = grad_loc_out; a.gattn_out = grad_attn_out;
    for (int i = 0; i < BEV_MAX_DEPTH; ++i)
        a.depth_base[i] = i < D ? depth_base[i] : 0.f;
    for (int i = 0; i < 6; ++i)
        a.pc[i] = pc_range[i];
    a.d_region = d_region;
    a.B = B; a.T = T; a.Q = Q; a.heads = heads; a.NP = NP; a.D = D; a.P = P; a.H = H; a.W = W;
    a.ld_off = ld_off; a.ld_ray = ld_ray; a.ld_scale = ld_scale; a.ld_queue = ld_queue;
    a.gld_off = gld_off; a.gld_ray = gld_ray; a.gld_scale = gld_scale; a.gld_queue = gld_queue;
    if (lds > 64 * 1024) {
        // (batch only) more dynamic LDS than a launch may ask for by default: raise the kernel's limit first
        const hipError_t e = hipFuncSetAttribute((const void *)bev_sampling_bwd_d64_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        RAC_CHECK_ARG(e == hipSuccess, "%s: %zu bytes of LDS per workgroup refused (%s)", fn, lds, hipGetErrorString(e));
    }
    if (batch)
        hipLaunchKernelGGL(bev_sampling_bwd_d64_kernel<false>, dim3(Q), dim3(256), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(bev_sampling_bwd_d64_kernel<true>, dim3(Q), dim3(256), lds, (hipStream_t)stream, a);
    return rac_launch_status(fn);
}

extern "C" int rac_bev_sampling_bwd(const void *value, const float *query_bbox, const float *box_table, const float *offsets,
                                    const float *ray_logits, const float *scale_logits, const float *queue_logits,
                                    const float *time_diff, const float *grad_out, float *grad_value, float *grad_offsets,
                                    float *grad_ray, float *grad_scale, float *grad_queue, float *grad_box, float *grad_loc_out,
                                    float *grad_attn_out, int ld_off, int ld_ray, int ld_scale, int ld_queue, int gld_off,
                                    int gld_ray, int gld_scale, int gld_queue, int B, int T, int Q, int heads, int NP, int D, int H,
                                    int W, int dim, const float *pc_range, const float *depth_base, float d_region, int dtype,
                                    void *stream)
{
    return bev_bwd_launch("rac_bev_sampling_bwd", false, value, query_bbox, box_table, offsets, ray_logits, scale_logits, queue_logits, time_diff, grad_out,
                          grad_value, grad_offsets, grad_ray, grad_scale, grad_queue, grad_box, grad_loc_out, grad_attn_out, ld_off, ld_ray,
                          ld_scale, ld_queue, gld_off, gld_ray, gld_scale, gld_queue, B, T, Q, heads, NP, D, H, W, dim, pc_range, depth_base,
                          d_region, dtype, stream);
}

extern "C" int rac_bev_sampling_bwd_batch(const void *value, const float *query_bbox, const float *box_table, const float *offsets,
                                          const float *ray_logits, const float *scale_logits, const float *queue_logits,
                                          const float *time_diff, const float *grad_out, float *grad_value, float *grad_offsets,
                                          float *grad_ray, float *grad_scale, float *grad_queue, float *grad_box, float *grad_loc_out,
                                          float *grad_attn_out, int ld_off, int ld_ray, int ld_scale, int ld_queue, int gld_off,
                                          int gld_ray, int gld_scale, int gld_queue, int B, int T, int Q, int heads, int NP, int D, int H,
                                          int W, int dim, const float *pc_range, const float *depth_base, float d_region, int dtype,
                                          void *stream)
{
    return bev_bwd_launch("rac_bev_sampling_bwd_batch", true, value, query_bbox, box_table, offsets, ray_logits, scale_logits, queue_logits, time_diff, grad_out,
                          grad_value, grad_offsets, grad_ray, grad_scale, grad_queue, grad_box, grad_loc_out, grad_attn_out, ld_off, ld_ray,
                          ld_scale, ld_queue, gld_off, gld_ray, gld_scale, gld_queue, B, T, Q, heads, NP, D, H, W, dim, pc_range, depth_base,
                          d_region, dtype, stream);
}
