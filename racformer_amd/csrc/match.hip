// match.hip -- the Hungarian assigners of the head loss on the device (gfx950): the match-cost matrices of all
// P = layers x samples problems in one launch, and their rectangular assignment problems in a second one.  Replaces, per
// (layer, sample), PolarHungarianAssigner3D.assign / HungarianAssigner3D.assign (models/bbox/assigners/*.py): ~15 torch
// launches for the cost, a blocking copy of the matrix to the host, scipy's linear_sum_assignment, a copy back.
//
// rac_match_cost_fwd   cost[p][g][q] = FocalLossCost + BBox3DL1Cost (+ ThetaL1Cost), nan_to_num(100, 100, -100); query index
//                      fastest (row pitch Qpad), so the solver reads a box's row coalesced.  Only g < G_b, q < Q is written.
// rac_lsap_fwd         shortest augmenting paths with duals in float64 (Jonker-Volgenant / Crouse 2016, what scipy implements);
//                      one wave64 per problem, no workgroup barrier: lane l owns the queries j = l (mod 64); each Dijkstra
//                      step relaxes the unscanned queries and takes a wave-wide (value, index) minimum, ties to the smaller
//                      index.  The working set (v, path lengths, u in float64; path, both matchings as 16-bit) lives in LDS.
#include "rac_common.h"

#define MATCH_MAX_B 64
#define MATCH_THREADS 256
#define LSAP_MAX_Q 2048

struct MatchArgs {
    const float *cls;      // [L][B][Q][C] logits
    const float *box;      // [L][B][Q][10]
    const float *gt;       // [sum G][9]: x, y, z, w, l, h, yaw, vx, vy
    const int *labels;     // [sum G]
    const float *cw;       // [10] code weights
    float *cost;           // [P][Gmax][Qpad]
    int off[MATCH_MAX_B + 1];
    int B, Q, C, Gmax, Qpad, polar;
    float w_cls, w_reg, w_theta;
};

// theta (turns) of a code-weighted centre, through ThetaL1Cost's own normalisation (pc_range -51.2 .. 51.2 whatever the config
// says: match_cost.py:50-56) and xy2theta_d_coods(norm=True) (bbox/utils.py:93-101)
__device__ __forceinline__ float match_theta(float x, float y)
{
    const float two_pi = 6.283185307179586f;
    const float nx = (x - (-51.2f)) / 102.4f, ny = (y - (-51.2f)) / 102.4f;
    const float dx = nx * 102.4f - 51.2f, dy = ny * 102.4f - 51.2f;
    return fmodf(atan2f(dy, dx) + two_pi, two_pi) / two_pi;
}

__global__ __launch_bounds__(MATCH_THREADS) void match_cost_kernel(const MatchArgs a)
{
    __shared__ float s_gt[MATCH_THREADS][11];   // code-weighted normalize_bbox(gt) (10), theta
    __shared__ int s_label[MATCH_THREADS];
    const int p = blockIdx.y, b = p % a.B;
    const int g0 = a.off[b], G = a.off[b + 1] - g0;
    const int q = blockIdx.x * MATCH_THREADS + threadIdx.x;
    const bool live = q < a.Q;
    float cw[10], pb[10];
#pragma unroll
    for (int k = 0; k < 10; ++k)
        cw[k] = a.cw[k];
    float theta_q = 0.f;
    const float *cls = a.cls + ((size_t)p * a.Q + (live ? q : 0)) * a.C;
    if (live) {
        const float *bx = a.box + ((size_t)p * a.Q + q) * 10;
#pragma unroll
        for (int k = 0; k < 10; ++k)
            pb[k] = bx[k] * cw[k];
        theta_q = match_theta(pb[0], pb[1]);
    }
    float *out = a.cost + (size_t)p * a.Gmax * a.Qpad;
    for (int base = 0; base < G; base += MATCH_THREADS) {
        const int n = min(MATCH_THREADS, G - base);
        __syncthreads();
        if ((int)threadIdx.x < n) {
            const float *t = a.gt + (size_t)(g0 + base + threadIdx.x) * 9;
            float nb[10] = {t[0], t[1], logf(t[3]), logf(t[4]), t[2], logf(t[5]), sinf(t[6]), cosf(t[6]), t[7], t[8]};
#pragma unroll
            for (int k = 0; k < 10; ++k)
                s_gt[threadIdx.x][k] = nb[k] * cw[k];
            s_gt[threadIdx.x][10] = match_theta(nb[0] * cw[0], nb[1] * cw[1]);
            s_label[threadIdx.x] = a.labels[g0 + base + threadIdx.x];
        }
        __syncthreads();
        if (!live)
            continue;
        for (int gi = 0; gi < n; ++gi) {
            const int label = s_label[gi];
            float c;
            if (label >= 0 && label < a.C) {
                // FocalLossCost (alpha 0.25, gamma 2, eps 1e-12)
                const float x = cls[label];
                const float pr = 1.f / (1.f + expf(-x));
                const float neg = -logf(1.f - pr + 1e-12f) * 0.75f * (pr * pr);
                const float pos = -logf(pr + 1e-12f) * 0.25f * ((1.f - pr) * (1.f - pr));
                c = (pos - neg) * a.w_cls;
            } else {
                c = __builtin_nanf("");     // (a label outside the classes: the reference's indexing would raise)
            }
            float l1 = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k)
                l1 += fabsf(pb[k] - s_gt[gi][k]);
            c += l1 * a.w_reg;
            if (a.polar) {
                const float d = fabsf(theta_q - s_gt[gi][10]);
                float r = fmodf(d + 0.5f, 1.f);         // (d >= 0: torch.remainder is fmod here)
                c += fabsf(r - 0.5f) * a.w_theta;
            }
            if (c != c)
                c = 100.f;
            else if (c == __builtin_inff())
                c = 100.f;
            else if (c == -__builtin_inff())
                c = -100.f;
            out[(size_t)(base + gi) * a.Qpad + q] = c;
        }
    }
}

extern "C" int rac_match_cost_fwd(const float *cls_scores, const float *bbox_preds, const float *gt_boxes, const int32_t *gt_labels,
                                  const int32_t *offsets, const float *code_weights, float *cost, int num_layers, int batch,
                                  int num_query, int num_classes, int gmax, int qpad, float cls_weight, float reg_weight,
                                  float theta_weight, int polar, void *stream)
{
    RAC_CHECK_ARG(num_layers >= 1 && batch >= 1 && batch <= MATCH_MAX_B && num_query >= 1 && num_classes >= 1,
                  "rac_match_cost_fwd: L=%d B=%d (1..%d) Q=%d C=%d", num_layers, batch, MATCH_MAX_B, num_query, num_classes);
    RAC_CHECK_ARG(gmax >= 0 && qpad >= num_query, "rac_match_cost_fwd: gmax=%d qpad=%d (>= Q=%d)", gmax, qpad, num_query);
    RAC_CHECK_ARG(offsets, "rac_match_cost_fwd: null pointer");
    MatchArgs a;
    for (int b = 0; b <= batch; ++b)
        a.off[b] = offsets[b];
    RAC_CHECK_ARG(a.off[0] == 0, "rac_match_cost_fwd: offsets[0] = %d", a.off[0]);
    for (int b = 0; b < batch; ++b)
        RAC_CHECK_ARG(a.off[b + 1] >= a.off[b] && a.off[b + 1] - a.off[b] <= gmax, "rac_match_cost_fwd: sample %d has %d boxes (0..gmax=%d)",
                      b, a.off[b + 1] - a.off[b], gmax);
    if (gmax == 0)
        return 0;
    RAC_CHECK_ARG(cls_scores && bbox_preds && gt_boxes && gt_labels && code_weights && cost, "rac_match_cost_fwd: null pointer");
    a.cls = cls_scores; a.box = bbox_preds; a.gt = gt_boxes; a.labels = gt_labels; a.cw = code_weights; a.cost = cost;
    a.B = batch; a.Q = num_query; a.C = num_classes; a.Gmax = gmax; a.Qpad = qpad; a.polar = polar;
    a.w_cls = cls_weight; a.w_reg = reg_weight; a.w_theta = theta_weight;
    hipLaunchKernelGGL(match_cost_kernel, dim3((num_query + MATCH_THREADS - 1) / MATCH_THREADS, num_layers * batch), dim3(MATCH_THREADS), 0,
                       (hipStream_t)stream, a);
    return rac_launch_status("rac_match_cost_fwd");
}

// ------------------------------------------------------------------------------------------------------------ assignment
struct LsapArgs {
    const float *cost;     // [P][Gmax][Qpad]
    int *matched_query;    // [P][Gmax]: the query of box g, -1 beyond G_b
    int *assigned_gt;      // [P][Q]: off[b] + g, or -1
    double *u;             // [P][Gmax]
    double *v;             // [P][Q]
    int *steps;            // [P] Dijkstra steps, or NULL
    int off[MATCH_MAX_B + 1];
    int B, Q, Gmax, Qpad;
};

// lanes of the one wave hand values to each other through LDS: program order is execution order within a wave, so all it takes
// is that the compiler keeps the accesses on their side of this point
#define LSAP_SYNC()                                          \
    do {                                                     \
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); \
        __builtin_amdgcn_wave_barrier();                     \
    } while (0)

__device__ __forceinline__ void lsap_wave_min(double &val, int &idx)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const double ov = __shfl_xor(val, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        if (ov < val || (ov == val && oi < idx)) {
            val = ov;
            idx = oi;
        }
    }
}

__global__ __launch_bounds__(64) void lsap_kernel(const LsapArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lsap_lds[];
    const int Q = a.Q, Qr = (Q + 63) & ~63;
    // carve: three float64 arrays first (8-byte aligned), then the 16-bit ones
    double *v = reinterpret_cast<double *>(lsap_lds);
    double *shortest = v + Qr;
    double *u = shortest + Qr;                                      // [Gr]
    const int p = blockIdx.x, b = p % a.B, lane = threadIdx.x;
    const int G = a.off[b + 1] - a.off[b], Gr = (a.Gmax + 63) & ~63;
    unsigned short *path = reinterpret_cast<unsigned short *>(u + Gr);   // [Qr] the row a column's shortest path comes from
    short *row4col = reinterpret_cast<short *>(path + Qr);               // [Qr]
    short *col4row = row4col + Qr;                                       // [Gr]
    unsigned char *scanned = reinterpret_cast<unsigned char *>(col4row + Gr);   // [Qr]
    const double inf = __builtin_inf();
    const float *cost = a.cost + (size_t)p * a.Gmax * a.Qpad;

    for (int j = lane; j < Qr; j += 64) {
        v[j] = 0.0;
        row4col[j] = -1;
    }
    for (int g = lane; g < Gr; g += 64) {
        u[g] = 0.0;
        col4row[g] = -1;
    }
    LSAP_SYNC();
    int steps = 0;
    bool failed = false;
    for (int cur = 0; cur < G && !failed; ++cur) {
        for (int j = lane; j < Qr; j += 64) {
            shortest[j] = inf;
            scanned[j] = 0;
        }
        double min_val = 0.0;
        int i = cur, sink = -1;
        // every step scans one more query: at most Q steps
        for (int step = 0; step < Q && sink < 0; ++step) {
            const float *row = cost + (size_t)i * a.Qpad;
            const double ui = u[i];
            double lowest = inf;
            int index = 0x7fffffff;
            for (int j = lane; j < Q; j += 64) {
                if (scanned[j])
                    continue;
                const double r = min_val + (double)row[j] - ui - v[j];
                double s = shortest[j];
                if (r < s) {
                    s = r;
                    shortest[j] = r;
                    path[j] = (unsigned short)i;
                }
                if (s < lowest) {           // (j ascends within a lane: strict, so the smaller index keeps a tie)
                    lowest = s;
                    index = j;
                }
            }
            lsap_wave_min(lowest, index);
            ++steps;
            if (index >= Q || !(lowest < inf)) {     // no finite entry left (NaN or +inf costs): give the problem up
                failed = true;
                break;
            }
            min_val = lowest;
            const int r4c = row4col[index];
            if (lane == 0)
                scanned[index] = 1;
            if (r4c < 0)
                sink = index;
            else
                i = r4c;
            LSAP_SYNC();
        }
        if (sink < 0) {
            failed = true;
            break;
        }
        // duals: u of the rows reached (cur, and the row of every scanned assigned query), v of the scanned queries
        for (int j = lane; j < Q; j += 64) {
            if (!scanned[j])
                continue;
            const double d = min_val - shortest[j];
            if (j != sink)
                u[row4col[j]] += d;        // (distinct rows: a matching)
            v[j] -= d;
        }
        LSAP_SYNC();
        if (lane == 0) {
            u[cur] += min_val;
            int j = sink;
            for (int hop = 0; hop <= G; ++hop) {        // (a path visits each row at most once)
                const int r = path[j];
                row4col[j] = (short)r;
                const int prev = col4row[r];
                col4row[r] = (short)j;
                j = prev;
                if (r == cur)
                    break;
            }
        }
        LSAP_SYNC();
    }
    // a problem given up is reported as unmatched throughout
    for (int g = lane; g < a.Gmax; g += 64) {
        a.matched_query[(size_t)p * a.Gmax + g] = (g < G && !failed) ? (int)col4row[g] : -1;
        a.u[(size_t)p * a.Gmax + g] = (g < G && !failed) ? u[g] : 0.0;
    }
    for (int j = lane; j < Q; j += 64) {
        const int r = failed ? -1 : (int)row4col[j];
        a.assigned_gt[(size_t)p * Q + j] = r < 0 ? -1 : a.off[b] + r;
        a.v[(size_t)p * Q + j] = failed ? 0.0 : v[j];
    }
    if (a.steps && lane == 0)
        a.steps[p] = failed ? -steps : steps;
}

extern "C" int rac_lsap_fwd(const float *cost, const int32_t *offsets, int32_t *matched_query, int32_t *assigned_gt, double *u, double *v,
                            int32_t *steps, int num_layers, int batch, int num_query, int gmax, int qpad, void *stream)
{
    RAC_CHECK_ARG(num_layers >= 1 && batch >= 1 && batch <= MATCH_MAX_B, "rac_lsap_fwd: L=%d B=%d (1..%d)", num_layers, batch, MATCH_MAX_B);
    RAC_CHECK_ARG(num_query >= 1 && qpad >= num_query && gmax >= 0, "rac_lsap_fwd: Q=%d qpad=%d gmax=%d", num_query, qpad, gmax);
    RAC_CHECK_ARG(offsets && assigned_gt && v, "rac_lsap_fwd: null pointer");
    RAC_CHECK_ARG(gmax == 0 || (cost && matched_query && u), "rac_lsap_fwd: null pointer");
    if (num_query > LSAP_MAX_Q || gmax > num_query) {
        rac_set_error("rac_lsap_fwd: Q=%d (<= %d), gmax=%d (<= Q): larger problems take rac_lsap_host", num_query, LSAP_MAX_Q, gmax);
        return RAC_E_UNSUPPORTED;
    }
    LsapArgs a;
    for (int b = 0; b <= batch; ++b)
        a.off[b] = offsets[b];
    RAC_CHECK_ARG(a.off[0] == 0, "rac_lsap_fwd: offsets[0] = %d", a.off[0]);
    for (int b = 0; b < batch; ++b)
        RAC_CHECK_ARG(a.off[b + 1] >= a.off[b] && a.off[b + 1] - a.off[b] <= gmax, "rac_lsap_fwd: sample %d has %d boxes (0..gmax=%d)", b,
                      a.off[b + 1] - a.off[b], gmax);
    a.cost = cost; a.matched_query = matched_query; a.assigned_gt = assigned_gt; a.u = u; a.v = v; a.steps = steps;
    a.B = batch; a.Q = num_query; a.Gmax = gmax; a.Qpad = qpad;
    const int Qr = (num_query + 63) & ~63, Gr = (gmax + 63) & ~63;
    const size_t lds = (size_t)(2 * Qr + Gr) * 8 + (size_t)(2 * Qr + Gr) * 2 + (size_t)Qr;      // 63488 bytes at Q = G = 2048
    hipLaunchKernelGGL(lsap_kernel, dim3(num_layers * batch), dim3(64), lds, (hipStream_t)stream, a);
    return rac_launch_status("rac_lsap_fwd");
}
