// sampling_fused_bwd.hip -- backward of rac_sampling4d_fwd (sampling_fused.hip) as ONE kernel (gfx950): float32 features.
//
// Forward, per (b, q), frame t, group g, point p and channel c:
//   out[b,q,g,t*P+p,c] = sum_l wl[l] * bilinear(feat_l[(b,t,g)][view], (u, v))[c]
// with wl = softmax_L(scale logits of slot (g', t'), quirk Q1), view the first camera of frame t that sees the point, and (u, v)
// the keypoint chain of s4d_keypoint:
//   base   = centre + R(yaw) (wlh * offset[g,p])                               (T-invariant; box table of rac_box_prep_fwd)
//   (X, Y) = clamp01(polar_jitter(warp(base - vel * time_diff[t]), doff[p % D])),  z = base z
//   (u, v) = (cam x, cam y) / max(homo, eps) / (image_w, image_h)              (lidar2img row of (t, view))
// Nothing of the forward is saved.  Everything discrete or weight-bearing -- location, camera, level weights, tap offsets -- comes
// from the forward's own device functions (s4d_keypoint, s4d_taps_of_level), called unchanged in a loop of their own, so the
// locations are the forward's bits; the derivative factors of the chain tail are recomputed here.
//
// Workgroup = one (b, q), 256 threads, walking the query's T*G*P keypoints, so every sum over frames, groups and points has one writer:
//   phase 1  one thread per keypoint (t, g, p): s4d_keypoint -> location, camera and level weights into LDS;
//   phase 2  the gather half, as rac_msmv_bwd: a 16-lane group per keypoint, lane c owns channels c + 16 j; per level the four
//            taps of s4d_taps_of_level: feature taps loaded, grad_feats scattered with float atomics (whole 64-byte segments),
//            the channel sums (d/d wl, d/d u, d/d v) by a butterfly inside the group; lane 0 keeps them in LDS;
//   phase 3  the chain tail, one thread per keypoint: projection, clamps, polar jitter and warp backwards -> d/d base point,
//            d/d range; softmax backwards over L -> grad_scale at the slot the forward read;
//   phase 4  fixed-order sums: over frames -> offsets; over frames, groups and points -> ray logits; over everything -> box table.
// Everything except grad_feats is written once, from sums in a fixed order (bit-reproducible).  Velocity, time_diff and
// lidar2img get no gradient (the reference detaches the velocity).
#include "s4d_device.h"
#include "gather_device.h"

struct S4dBwdArgs {
    S4dArgs f;                       // the forward's arguments (out unused; loc_out / w_out: the recomputed keypoints, debug)
    const float *grad_out;           // [B,Q,G,T*P,64]
    float *gfeat[RAC_MAX_LEVELS];    // as feat[l], zero-filled by the caller (all null: no feature gradient wanted)
    float *goff, *gray, *gscale;     // rows (gld_*)
    float *gbox;                     // [B,Q,8]
    float *gloc_out, *gw_out;        // optional [S,Q,P,2] / [S,Q,P,L]
    int gld_off, gld_ray, gld_scale;
    int scatter;                     // 1: grad_feats wanted
};

// LDS floats: per keypoint 5 + 2 L (u -> d/d x; v -> d/d y; d/d u -> d/d z; d/d v -> d/d range; camera; wl[L]; d/d wl[L]), the
// frames' projection matrices, per (g, p) 6 (offsets as read, frame sums of d/d base point), box row + velocity, sigmoids
static size_t s4d_bwd_lds_floats(int L, int T, int N, int G, int P)
{
    return (size_t)T * G * P * (5 + 2 * L) + (size_t)T * N * 16 + (size_t)G * P * 6 + 16 + S4D_MAX_DEPTH;
}

// Backward of the chain of s4d_keypoint at one keypoint, from the gradient (gu, gv) of its image location in camera matrix m
// (the selected view's) down to the base point (res[0..2]: x, y, z) and the range jitter (res[3]).  bx: box-table row [0..7] and
// velocity [8..9]; (o0, o1, o2): the point's offset; td: time_diff[t]; doff: depth_base + jitter of the point's depth slot.
// homo passes the gradient only where homo > eps (torch.maximum); the two clamps inside [0,1] inclusive (torch.clamp).
// The gates are discrete and are taken from THIS float32 restatement of the chain, which the compiler may contract differently
// from s4d_keypoint: at a keypoint within a rounding of a gate (ux or uy at 0 or 1, homo at eps) the backward's gate can differ
// from the forward's.  The forward's value is continuous across the two clamps, and across homo = eps up to eps itself, so the
// gradient returned there is the derivative of one side.
__device__ __forceinline__ void s4d_tail_bwd(const S4dArgs &a, const float *m, const float *bx, float o0, float o1, float o2,
                                             float td, float doff, float gu, float gv, float *res)
{
    const float sx = a.pc[3] - a.pc[0], sy = a.pc[4] - a.pc[1];
    const float cs = bx[6], sn = bx[7];
    const float dx = bx[3] * o0, dy = bx[4] * o1, dz = bx[5] * o2;
    const float px = bx[0] + (dx * cs - dy * sn) - bx[8] * td;
    const float py = bx[1] + (dx * sn + dy * cs) - bx[9] * td;
    const float pz = bx[2] + dz;
    const float nx = (px - a.pc[0]) / sx, ny = (py - a.pc[1]) / sy;
    const float ex = nx * 102.4f - 51.2f, ey = ny * 102.4f - 51.2f;
    const float r2 = ex * ex + ey * ey, r = sqrtf(r2);
    const float dist = r / 65.0f + doff;
    const float th = fmodf(atan2f(ey, ex) + S4D_TWO_PI, S4D_TWO_PI) / S4D_TWO_PI;
    const float ang = th * S4D_TWO_PI, rad = dist * 65.0f;
    const float ca = cosf(ang), sa = sinf(ang);
    const float ux = (51.2f + rad * ca) / 102.4f, uy = (51.2f + rad * sa) / 102.4f;
    const float X = fminf(fmaxf(ux, 0.f), 1.f) * sx + a.pc[0];
    const float Y = fminf(fmaxf(uy, 0.f), 1.f) * sy + a.pc[1];
    const float camx = m[0] * X + m[1] * Y + m[2] * pz + m[3];
    const float camy = m[4] * X + m[5] * Y + m[6] * pz + m[7];
    const float homo = m[8] * X + m[9] * Y + m[10] * pz + m[11];
    const float hz = fmaxf(homo, a.eps);
    // u = camx / hz / image_w, v = camy / hz / image_h
    const float g_camx = gu / (hz * a.image_w), g_camy = gv / (hz * a.image_h);
    const float g_homo = homo > a.eps ? -(g_camx * camx + g_camy * camy) / hz : 0.f;
    const float gX = m[0] * g_camx + m[4] * g_camy + m[8] * g_homo;
    const float gY = m[1] * g_camx + m[5] * g_camy + m[9] * g_homo;
    res[2] = m[2] * g_camx + m[6] * g_camy + m[10] * g_homo;
    const float gux = (ux >= 0.f && ux <= 1.f) ? gX * sx / 102.4f : 0.f;
    const float guy = (uy >= 0.f && uy <= 1.f) ? gY * sy / 102.4f : 0.f;
    const float g_rad = gux * ca + guy * sa;               // = d/d r (dist = r / 65 + doff, rad = 65 dist)
    const float g_ang = rad * (guy * ca - gux * sa);       // = d/d atan2 (the fmod and the two 2 pi factors have slope 1)
    // r = 0 (a point on the map centre): sqrt and atan2 have no derivative there; no gradient to the base point
    const float ir = r2 > 0.f ? 1.f / r : 0.f, ir2 = r2 > 0.f ? 1.f / r2 : 0.f;
    const float g_ex = g_rad * ex * ir - g_ang * ey * ir2;
    const float g_ey = g_rad * ey * ir + g_ang * ex * ir2;
    res[0] = g_ex * 102.4f / sx;
    res[1] = g_ey * 102.4f / sy;
    res[3] = g_rad * 65.0f;
}

template <int L>
__global__ __launch_bounds__(256) void sampling4d_bwd_c64_kernel(const S4dBwdArgs A)
{
    const S4dArgs &a = A.f;
    extern __shared__ float smem[];
    const int tid = threadIdx.x;
    const int b = blockIdx.x / a.Q, q = blockIdx.x - b * a.Q;
    const int T = a.T, G = a.G, P = a.P, N = a.N, D = a.D, GP = G * P, K = T * GP;
    // keypoint index k = (t * G + g) * P + p: frame-major, as the forward's slots
    float *ku = smem;                 // [K] u                     -> phase 3: d/d base x
    float *kv = ku + K;               // [K] v                     -> phase 3: d/d base y
    float *kgu = kv + K;              // [K] d/d u                 -> phase 3: d/d base z
    float *kgv = kgu + K;             // [K] d/d v                 -> phase 3: d/d range
    float *kwl = kgv + K;             // [K][L] level weights
    float *kgw = kwl + K * L;         // [K][L] d/d level weight
    int *kview = reinterpret_cast<int *>(kgw + K * L);          // [K] camera sampled
    float *sl2i = reinterpret_cast<float *>(kview + K);         // [T][N][16]
    float *soff = sl2i + T * N * 16;  // [GP][3] the offsets as read
    float *sgb = soff + GP * 3;       // [GP][3] sum over frames of d/d base point
    float *sbox = sgb + GP * 3;       // [8] box table row, [8..9] velocity
    float *ssig = sbox + 16;          // [S4D_MAX_DEPTH] sigmoid(ray)

    const size_t bq = (size_t)b * a.Q + q;
    for (int i = tid; i < T * N * 16; i += 256)
        sl2i[i] = a.l2i[(size_t)b * T * N * 16 + i];
    if (tid < 8)
        sbox[tid] = a.box[bq * 8 + tid];
    if (tid >= 8 && tid < 10)
        sbox[tid] = a.qbox[bq * 10 + tid];
    for (int i = tid; i < GP * 3; i += 256)
        soff[i] = a.off[bq * a.ld_off + i];
    if (tid >= 128 && tid < 128 + D)
        ssig[tid - 128] = 1.f / (1.f + expf(-a.ray[bq * a.ld_ray + tid - 128]));
    __syncthreads();
    // phase 1: keypoints, the forward's prologue
    for (int k = tid; k < K; k += 256) {
        const int t = k / GP, gp = k - t * GP, g = gp / P, p = gp - g * P;
        float loc3[3], wl[L];
        s4d_keypoint<L>(a, sl2i + t * N * 16, b, t, g, q, p, loc3, wl);
        ku[k] = loc3[0];
        kv[k] = loc3[1];
        kview[k] = (int)loc3[2] & 255;
#pragma unroll
        for (int l = 0; l < L; ++l)
            kwl[k * L + l] = wl[l];
        if (a.loc_out) {
            const size_t e = ((((size_t)b * T + t) * G + g) * a.Q + q) * P + p;
            a.loc_out[e * 3] = loc3[0];
            a.loc_out[e * 3 + 1] = loc3[1];
            a.loc_out[e * 3 + 2] = (float)((int)loc3[2] >> 8) / (float)max(N - 1, 1);
#pragma unroll
            for (int l = 0; l < L; ++l)
                a.w_out[e * L + l] = wl[l];
        }
    }
    __syncthreads();
    // phase 2: gather half.  16 groups of 16 lanes; group i takes keypoints i, i + 16, ...
    {
        const int lane16 = tid & 15, grp = tid >> 4;
        for (int k = grp; k < K; k += 16) {
            const int t = k / GP, gp = k - t * GP, g = gp / P, p = gp - g * P;
            const size_t s = ((size_t)b * T + t) * G + g;
            const float lu = ku[k], lv = kv[k];
            const int view = kview[k];
            const bool view_ok = view < N;      // (an imposed camera index beyond the rig: no taps)
            const float *go = A.grad_out + ((((bq * G + g) * T + t) * P + p) * 64 + lane16);
            float gch[4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                gch[j] = go[16 * j];
            float gu = 0.f, gv = 0.f, gwl[L];
#pragma unroll
            for (int l = 0; l < L; ++l) {
                const int H = a.H[l], W = a.W[l];
                const float wl = kwl[k * L + l];
                alignas(16) float e[8];
                s4d_taps_of_level<float>(H, W, lu, lv, view, wl, 0u, e);
                const s4d_u4 o4 = *reinterpret_cast<const s4d_u4 *>(e);
                const unsigned o[4] = {o4.x, o4.y, o4.z, o4.w};
                const RacFootprint f = rac_footprint(lv * (float)(H - 1), lu * (float)(W - 1), H, W);
                const float lh = f.lh, lw = f.lw, hh = f.hh, hw = f.hw;
                const float tw[4] = {hh * hw, hh * lw, lh * hw, lh * lw};
                const float dh[4] = {-hw, -lw, hw, lw}, dw[4] = {-hh, hh, -lh, lh};
                const char *base = reinterpret_cast<const char *>(a.feat[l]) + s * a.feat_bytes[l];
                char *gbase = reinterpret_cast<char *>(A.gfeat[l]) + s * a.feat_bytes[l];
                float sv = 0.f, sh = 0.f, sw_ = 0.f;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const bool ok = view_ok && o[c] != S4D_TAP_OUTSIDE;
                    float v[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        v[j] = ok ? reinterpret_cast<const float *>(base + o[c])[lane16 + 16 * j] : 0.f;
                    if (ok && A.scatter) {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            atomicAdd(reinterpret_cast<float *>(gbase + o[c]) + lane16 + 16 * j, e[4 + c] * gch[j]);
                    }
                    const float dot = (v[0] * gch[0] + v[1] * gch[1]) + (v[2] * gch[2] + v[3] * gch[3]);
                    sv += tw[c] * dot;
                    sh += dh[c] * dot;
                    sw_ += dw[c] * dot;
                }
                sv = rac_group_sum16(sv);
                sh = rac_group_sum16(sh);
                sw_ = rac_group_sum16(sw_);
                gwl[l] = f.in ? sv : 0.f;
                gu += (float)(W - 1) * sw_ * wl;
                gv += (float)(H - 1) * sh * wl;
            }
            if (lane16 == 0) {
                kgu[k] = gu;
                kgv[k] = gv;
#pragma unroll
                for (int l = 0; l < L; ++l)
                    kgw[k * L + l] = gwl[l];
                const size_t e = (s * a.Q + q) * P + p;
                if (A.gloc_out) {
                    A.gloc_out[e * 2] = gu;
                    A.gloc_out[e * 2 + 1] = gv;
                }
                if (A.gw_out) {
#pragma unroll
                    for (int l = 0; l < L; ++l)
                        A.gw_out[e * L + l] = gwl[l];
                }
            }
        }
    }
    __syncthreads();
    // phase 3: chain tail per keypoint; softmax over levels backwards into the (g', t') slot the forward read (quirk Q1: a bijection)
    for (int k = tid; k < K; k += 256) {
        const int t = k / GP, gp = k - t * GP, g = gp / P, p = gp - g * P;
        const int dd = p % D;
        const float doff = a.depth_base[dd] + (ssig[dd] * 2.f - 1.f) * a.d_region / (float)D / 2.f;
        const int view = min(kview[k], N - 1);
        float res[4];
        s4d_tail_bwd(a, sl2i + (t * N + view) * 16, sbox, soff[gp * 3], soff[gp * 3 + 1], soff[gp * 3 + 2],
                     a.time_diff[b * T + t], doff, kgu[k], kgv[k], res);
        ku[k] = res[0];
        kv[k] = res[1];
        kgu[k] = res[2];
        kgv[k] = res[3];
        float dot = 0.f;
#pragma unroll
        for (int l = 0; l < L; ++l)
            dot += kwl[k * L + l] * kgw[k * L + l];
        const int sp = t * G + g;
        const int gq = sp / T, tq = sp - gq * T;
        float *gs = A.gscale + bq * A.gld_scale + (((size_t)gq * T + tq) * P + p) * L;
#pragma unroll
        for (int l = 0; l < L; ++l)
            gs[l] = kwl[k * L + l] * (kgw[k * L + l] - dot);
    }
    __syncthreads();
    // phase 4a: sums over frames per (g, p) -> offsets; d/d range per depth slot -> ray logits.  Fixed order.
    const float bw = sbox[3], bl = sbox[4], bh = sbox[5], bcs = sbox[6], bsn = sbox[7];
    for (int i = tid; i < GP; i += 256) {
        float gx = 0.f, gy = 0.f, gz = 0.f;
        for (int t = 0; t < T; ++t) {
            gx += ku[t * GP + i];
            gy += kv[t * GP + i];
            gz += kgu[t * GP + i];
        }
        sgb[i * 3] = gx;
        sgb[i * 3 + 1] = gy;
        sgb[i * 3 + 2] = gz;
        float *gof = A.goff + bq * A.gld_off + (size_t)i * 3;
        gof[0] = bw * (gx * bcs + gy * bsn);
        gof[1] = bl * (gy * bcs - gx * bsn);
        gof[2] = bh * gz;
    }
    if (tid >= 128 && tid < 128 + D) {
        const int dd = tid - 128;
        float gd = 0.f;
        for (int tg = 0; tg < T * G; ++tg)
            for (int p = dd; p < P; p += D)
                gd += kgv[tg * P + p];
        const float sgm = ssig[dd];
        A.gray[bq * A.gld_ray + dd] = gd * (sgm * (1.f - sgm)) * 2.f * a.d_region / (float)D / 2.f;
    }
    __syncthreads();
    // phase 4b: box table (all eight entries: z, h and the rotation act through the projection)
    if (tid >= 64 && tid < 72) {
        const int e = tid - 64;
        float s = 0.f;
        for (int i = 0; i < GP; ++i) {
            const float gx = sgb[i * 3], gy = sgb[i * 3 + 1], gz = sgb[i * 3 + 2];
            const float o0 = soff[i * 3], o1 = soff[i * 3 + 1], o2 = soff[i * 3 + 2];
            const float dx = bw * o0, dy = bl * o1;
            float term;
            if (e == 0) term = gx;
            else if (e == 1) term = gy;
            else if (e == 2) term = gz;
            else if (e == 3) term = o0 * (gx * bcs + gy * bsn);
            else if (e == 4) term = o1 * (gy * bcs - gx * bsn);
            else if (e == 5) term = o2 * gz;
            else if (e == 6) term = gx * dx + gy * dy;
            else term = gy * dx - gx * dy;
            s += term;
        }
        A.gbox[bq * 8 + e] = s;
    }
}

extern "C" int rac_sampling4d_bwd(const void *const *feats, const int32_t *hw, int L, const float *query_bbox,
                                  const float *box_table, const float *offsets, const float *ray_logits,
                                  const float *scale_logits, const float *time_diff, const float *lidar2img,
                                  const unsigned char *view_in, const float *grad_out, void *const *grad_feats,
                                  float *grad_offsets, float *grad_ray, float *grad_scale, float *grad_box, float *grad_loc_out,
                                  float *grad_w_out, float *loc_out, float *w_out, int ld_off, int ld_ray, int ld_scale,
                                  int gld_off, int gld_ray, int gld_scale, int B, int T, int N, int G, int Q, int NP, int D, int C,
                                  const float *pc_range, const float *depth_base, float d_region, float image_h, float image_w,
                                  float eps, int dtype, void *stream)
{
    RAC_CHECK_ARG(L == 1 || L == 2 || L == 4 || L == 5, "rac_sampling4d_bwd: L=%d (supported: 1, 2, 4, 5)", L);
    RAC_CHECK_ARG(C == 64, "rac_sampling4d_bwd: C=%d (the fused kernel is built for 64 channels per group)", C);
    RAC_CHECK_ARG(B >= 0 && Q >= 0 && T >= 1 && N >= 1 && N <= S4D_MAX_CAMS && G >= 1 && NP >= 1 && D >= 1 &&
                      D <= S4D_MAX_DEPTH,
                  "rac_sampling4d_bwd: bad sizes B=%d T=%d N=%d G=%d Q=%d NP=%d D=%d", B, T, N, G, Q, NP, D);
    const int P = NP * D;
    RAC_CHECK_ARG(P <= RAC_MAX_POINTS, "rac_sampling4d_bwd: num_point exceed limits (P=%d > %d)", P, RAC_MAX_POINTS);
    RAC_CHECK_ARG(dtype == RAC_F32, "rac_sampling4d_bwd: dtype %d (float32 features only)", dtype);
    RAC_CHECK_ARG(ld_off >= G * P * 3 && ld_ray >= D && ld_scale >= G * T * P * L,
                  "rac_sampling4d_bwd: row strides ld_off=%d ld_ray=%d ld_scale=%d narrower than their rows", ld_off, ld_ray, ld_scale);
    RAC_CHECK_ARG(gld_off >= G * P * 3 && gld_ray >= D && gld_scale >= G * T * P * L,
                  "rac_sampling4d_bwd: gradient row strides gld_off=%d gld_ray=%d gld_scale=%d narrower than their rows", gld_off,
                  gld_ray, gld_scale);
    const size_t lds = s4d_bwd_lds_floats(L, T, N, G, P) * sizeof(float);
    RAC_CHECK_ARG(lds <= 64 * 1024, "rac_sampling4d_bwd: T*G*NP*D=%d keypoints per query x L=%d too many for the LDS staging", T * G * P, L);
    if (B == 0 || Q == 0)
        return 0;
    RAC_CHECK_ARG(box_table != nullptr, "rac_sampling4d_bwd: box_table is null (run rac_box_prep_fwd first)");
    RAC_CHECK_ARG(feats && hw && query_bbox && offsets && ray_logits && scale_logits && time_diff && lidar2img && grad_out &&
                      grad_offsets && grad_ray && grad_scale && grad_box && pc_range && depth_base,
                  "rac_sampling4d_bwd: null pointer");
    RAC_CHECK_ARG((loc_out == nullptr) == (w_out == nullptr), "rac_sampling4d_bwd: loc_out and w_out go together");
    S4dBwdArgs A;
    S4dArgs &a = A.f;
    for (int l = 0; l < RAC_MAX_LEVELS; ++l) {
        a.feat[l] = nullptr;
        A.gfeat[l] = nullptr;
        a.H[l] = a.W[l] = 1;
        a.feat_bytes[l] = 0;
    }
    for (int l = 0; l < L; ++l) {
        RAC_CHECK_ARG(feats[l] != nullptr && (!grad_feats || grad_feats[l] != nullptr) && hw[2 * l] >= 1 && hw[2 * l + 1] >= 1,
                      "rac_sampling4d_bwd: level %d", l);
        a.feat[l] = feats[l];
        A.gfeat[l] = grad_feats ? (float *)grad_feats[l] : nullptr;
        a.H[l] = hw[2 * l];
        a.W[l] = hw[2 * l + 1];
        const size_t bytes = (size_t)N * a.H[l] * a.W[l] * 64 * 4;      // one slot's maps
        RAC_CHECK_ARG(bytes < (size_t)S4D_TAP_OUTSIDE, "rac_sampling4d_bwd: a slot of level %d holds %zu bytes (the tap offsets are 31-bit)", l, bytes);
        a.feat_bytes[l] = (unsigned)bytes;
    }
    a.qbox = query_bbox; a.box = box_table; a.off = offsets; a.ray = ray_logits; a.scale = scale_logits;
    a.time_diff = time_diff; a.l2i = lidar2img; a.out = nullptr; a.loc_out = loc_out; a.w_out = w_out; a.view_in = view_in;
    for (int i = 0; i < S4D_MAX_DEPTH; ++i)
        a.depth_base[i] = i < D ? depth_base[i] : 0.f;
    for (int i = 0; i < 6; ++i)
        a.pc[i] = pc_range[i];
    a.d_region = d_region; a.image_h = image_h; a.image_w = image_w; a.eps = eps;
    a.L = L; a.B = B; a.T = T; a.N = N; a.G = G; a.Q = Q; a.NP = NP; a.D = D; a.P = P;
    a.ld_off = ld_off; a.ld_ray = ld_ray; a.ld_scale = ld_scale;
    a.blocks_per_slot = 0; a.rows = 0;
    A.grad_out = grad_out;
    A.goff = grad_offsets; A.gray = grad_ray; A.gscale = grad_scale; A.gbox = grad_box;
    A.gloc_out = grad_loc_out; A.gw_out = grad_w_out;
    A.gld_off = gld_off; A.gld_ray = gld_ray; A.gld_scale = gld_scale;
    A.scatter = grad_feats != nullptr;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(B * Q));
    if (L == 1) hipLaunchKernelGGL(sampling4d_bwd_c64_kernel<1>, grid, dim3(256), lds, st, A);
    else if (L == 2) hipLaunchKernelGGL(sampling4d_bwd_c64_kernel<2>, grid, dim3(256), lds, st, A);
    else if (L == 4) hipLaunchKernelGGL(sampling4d_bwd_c64_kernel<4>, grid, dim3(256), lds, st, A);
    else hipLaunchKernelGGL(sampling4d_bwd_c64_kernel<5>, grid, dim3(256), lds, st, A);
    return rac_launch_status("rac_sampling4d_bwd");
}
