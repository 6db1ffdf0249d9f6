// sasa.hip -- scale-adaptive self-attention core as one kernel (gfx950).
//
// Replaces, per decoder layer, calc_bbox_dists (a [B,Q,Q] cdist), the [B*8,Q,Q] float mask, and
// nn.MultiheadAttention's QK^T / softmax / AV (models/racformer_transformer.py:296-335 over mmcv's
// MultiheadAttention wrapper): nothing of size Q x Q ever touches HBM.
//   logits[b,h,i,j] = (q_i / sqrt(d)) . k_j  -  ||c_i - c_j||_2 * tau[b,i,h]
//   out[b,i,h*d:(h+1)*d] = softmax_j(logits) @ v
// with c = box centres in metres (decode_bbox(theta_d2xy(query_bbox))[:2], :301-302,:325).
// in_proj / out_proj stay library GEMMs outside.
// Under the boolean [Q,Q] attn_mask of query denoising (:311-312; rac_sasa_fwd_mask / rac_sasa_bwd_mask) the mask comes in as
// bits, 32 keys to a word, shared by all batches and heads: the masked instantiations of the matrix-core kernels below (a
// template parameter; the unmasked instantiations are the kernels they were) and, for Q > 1024, a streaming matrix-core forward.
//
// Mapping: a workgroup = 16 query rows of one (batch, head); a 16-lane group owns a row.  K/V are
// streamed through LDS in 64-key tiles (next tile prefetched into registers while the current one
// is consumed; row stride 36 floats = conflict-free ds_read_b128); lane r of a row scores keys
// r, r+16, r+32, r+48 of the tile and folds them into its own online-softmax state (running max,
// sum, d-wide accumulator) with one rescale per 4 keys; the 16 partial states of a row are merged
// with a log-sum-exp butterfly over the 16 lanes.  Centres of all keys are computed once per
// workgroup into LDS.  fp32 throughout (exact-fp32 VALU; fp32 MFMA has the same rate on gfx950).
#include "rac_common.h"

#define SASA_D 32
#define SASA_ROWS 16
#define SASA_TWO_PI 6.283185307179586f

struct SasaArgs {
    const float *qkv;   // [B,Q,3,H,d]  (in_proj output)
    const float *tau;   // [B,Q,H], row stride ld_tau
    const float *qbox;  // [B,Q,10]
    const float *box;   // optional [B,Q,8] from rac_box_prep_fwd (cx, cy, ...): skips the trig prologue
    float *out;         // [B,Q,H*d]
    float *lse;         // optional [B,H,Q]: log-sum-exp of every query row's logits (rac_sasa_fwd_ex)
    float pc[6];
    int B, Q, H, ld_tau, ld_qkv;
    int row_blocks;
    const unsigned *mask;  // masked instantiations only: [Q][ld_mask] words, bit j&31 of word [i][j>>5] set = query i does not see key j
    int ld_mask;
};

#define SASA_TILE 64   /* keys per LDS tile */
#define SASA_KS 36     /* LDS row stride (floats): 16-byte aligned and conflict-free for ds_read_b128 */

__global__ __launch_bounds__(256) void sasa_d32_kernel(const SasaArgs a)
{
    extern __shared__ float smem[];
    float *scen = smem;                       // [Q][2] key centres (metres)
    float *sK = smem + 2 * ((a.Q + 1) & ~1);  // [64][36]
    float *sV = sK + SASA_TILE * SASA_KS;     // [64][36]
    const int tid = threadIdx.x;
    const int r = tid & 15, row = tid >> 4;
    int bid = blockIdx.x;
    const int rb = bid % a.row_blocks; bid /= a.row_blocks;
    const int h = bid % a.H;
    const int b = bid / a.H;
    const int Q = a.Q, H = a.H;
    const size_t tok = (size_t)b * Q;
    const int ld = a.ld_qkv;  // floats per token row (>= 3*H*d: qkv may be a column slice of a wider GEMM output)

    // K/V tile staging: thread -> (key = tid/4 (0..63), 2 float4 of K and 2 of V at columns (tid%4)*2..)
    const int sk = tid >> 2, sc = (tid & 3) * 2;
    rac_f4 pk[2], pv[2];
    auto prefetch = [&](int tile) {
        const int j = tile * SASA_TILE + sk;
        const int jj = j < Q ? j : Q - 1;
        const rac_f4 *kp = reinterpret_cast<const rac_f4 *>(a.qkv + (tok + jj) * ld + (H + h) * SASA_D);
        const rac_f4 *vp = reinterpret_cast<const rac_f4 *>(a.qkv + (tok + jj) * ld + (2 * H + h) * SASA_D);
        pk[0] = kp[sc]; pk[1] = kp[sc + 1];
        pv[0] = vp[sc]; pv[1] = vp[sc + 1];
    };
    prefetch(0);

    for (int j = tid; j < Q; j += 256) {
        const float *qb = a.qbox + ((size_t)b * Q + j) * 10;
        const float ang = qb[0] * SASA_TWO_PI, rad = qb[1] * 65.0f;
        const float xn = fminf(fmaxf((51.2f + rad * cosf(ang)) / 102.4f, 0.f), 1.f);
        const float yn = fminf(fmaxf((51.2f + rad * sinf(ang)) / 102.4f, 0.f), 1.f);
        scen[2 * j] = xn * (a.pc[3] - a.pc[0]) + a.pc[0];
        scen[2 * j + 1] = yn * (a.pc[4] - a.pc[1]) + a.pc[1];
    }

    const int i = rb * SASA_ROWS + row;
    const bool live = i < Q;
    const int ii = live ? i : Q - 1;
    const float scale = 0.17677669529663687f;  // sqrt(1/32) as torch computes math.sqrt(1.0/d)
    float q[SASA_D];
    {
        const rac_f4 *qp = reinterpret_cast<const rac_f4 *>(a.qkv + (tok + ii) * ld + h * SASA_D);
#pragma unroll
        for (int c = 0; c < SASA_D / 4; ++c) {
            const rac_f4 t = qp[c];
            q[4 * c] = t.x * scale; q[4 * c + 1] = t.y * scale; q[4 * c + 2] = t.z * scale; q[4 * c + 3] = t.w * scale;
        }
    }
    const float tau = a.tau[(tok + ii) * a.ld_tau + h];
    __syncthreads();  // centres visible
    const float cix = scen[2 * ii], ciy = scen[2 * ii + 1];

    float m = -INFINITY, l = 0.f;
    float acc[SASA_D];
#pragma unroll
    for (int c = 0; c < SASA_D; ++c)
        acc[c] = 0.f;

    const int ntiles = (Q + SASA_TILE - 1) / SASA_TILE;
    for (int tile = 0; tile < ntiles; ++tile) {
        // publish the prefetched tile, start fetching the next one
        *reinterpret_cast<rac_f4 *>(sK + sk * SASA_KS + sc * 4) = pk[0];
        *reinterpret_cast<rac_f4 *>(sK + sk * SASA_KS + sc * 4 + 4) = pk[1];
        *reinterpret_cast<rac_f4 *>(sV + sk * SASA_KS + sc * 4) = pv[0];
        *reinterpret_cast<rac_f4 *>(sV + sk * SASA_KS + sc * 4 + 4) = pv[1];
        __syncthreads();
        if (tile + 1 < ntiles)
            prefetch(tile + 1);
        // lane r scores keys r, r+16, r+32, r+48 of the tile
        float sc4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int kl = r + 16 * u, j = tile * SASA_TILE + kl;
            const rac_f4 *kp = reinterpret_cast<const rac_f4 *>(sK + kl * SASA_KS);
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < SASA_D / 4; ++c) {
                const rac_f4 kk = kp[c];
                s += q[4 * c] * kk.x + q[4 * c + 1] * kk.y + q[4 * c + 2] * kk.z + q[4 * c + 3] * kk.w;
            }
            const int jc = j < Q ? j : Q - 1;
            const float dx = cix - scen[2 * jc], dy = ciy - scen[2 * jc + 1];
            s += -sqrtf(dx * dx + dy * dy) * tau;
            sc4[u] = j < Q ? s : -INFINITY;
        }
        const float mn = fmaxf(fmaxf(m, fmaxf(sc4[0], sc4[1])), fmaxf(sc4[2], sc4[3]));
        if (mn > -INFINITY) {
            const float corr = (m == -INFINITY) ? 0.f : expf(m - mn);
            l *= corr;
#pragma unroll
            for (int c = 0; c < SASA_D; ++c)
                acc[c] *= corr;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float p = (sc4[u] == -INFINITY) ? 0.f : expf(sc4[u] - mn);
                l += p;
                const rac_f4 *vp = reinterpret_cast<const rac_f4 *>(sV + (r + 16 * u) * SASA_KS);
#pragma unroll
                for (int c = 0; c < SASA_D / 4; ++c) {
                    const rac_f4 vv = vp[c];
                    acc[4 * c] += p * vv.x; acc[4 * c + 1] += p * vv.y; acc[4 * c + 2] += p * vv.z; acc[4 * c + 3] += p * vv.w;
                }
            }
            m = mn;
        }
        __syncthreads();  // everyone done with this tile before it is overwritten
    }
    // merge the 16 lanes of the row: log-sum-exp butterfly
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) {
        const float mo = __shfl_xor(m, off, 16);
        const float lo = __shfl_xor(l, off, 16);
        const float mn = fmaxf(m, mo);
        const float ca = (m == -INFINITY) ? 0.f : expf(m - mn);
        const float cb = (mo == -INFINITY) ? 0.f : expf(mo - mn);
        l = l * ca + lo * cb;
#pragma unroll
        for (int c = 0; c < SASA_D; ++c) {
            const float ao = __shfl_xor(acc[c], off, 16);
            acc[c] = acc[c] * ca + ao * cb;
        }
        m = mn;
    }
    if (live) {
        if (a.lse && r == 0)
            a.lse[((size_t)b * H + h) * Q + i] = m + logf(l);
        // lane r writes channels 2r, 2r+1 (all lanes hold the merged state)
        const float inv = 1.f / l;
        float o0 = 0.f, o1 = 0.f;
#pragma unroll
        for (int c = 0; c < SASA_D / 2; ++c)
            if (c == r) {
                o0 = acc[2 * c];
                o1 = acc[2 * c + 1];
            }
        float2 o = make_float2(o0 * inv, o1 * inv);
        *reinterpret_cast<float2 *>(a.out + (tok + i) * (size_t)(H * SASA_D) + h * SASA_D + 2 * r) = o;
    }
}

// ---------------------------------------------------------------------------------------------------
// Matrix-core version (default): QK^T and PV on v_mfma_f32_16x16x4_f32 (exact fp32).
// Workgroup = 16 queries of one (batch, head); its 4 waves take the 16-key tiles round-robin.
//   S^T tile [16 keys x 16 queries] = K_tile (A operand) . Q^T (B operand): 8 MFMAs.  With the k index of
//   a group of four steps assigned as k = 16u + 4*lk + i (as in rowgemm.hip) every operand is a 16-byte load.
//   The accumulator then holds S^T[key = 4*lk + r][query = li] -- exactly the B-operand layout of the
//   second product O^T[32 ch x 16 queries] = V^T (A operand) . P^T (B operand), so the probabilities go
//   from the first product's accumulators into the second product's operands without leaving registers.
//   Softmax statistics are per query = per lane column: a register reduction, two DPP steps over lk and
//   one LDS exchange between the four waves.
typedef float sasa_f4 __attribute__((ext_vector_type(4)));
#define SASA_NT 16 /* key tiles per wave: Q <= 4*16*16 = 1024 */

// The centres (metres) of batch element b's Q boxes into LDS, by the workgroup's 256 threads: from the box table when there
// is one, else decode_bbox(theta_d2xy(query_bbox))[:2] here.
__device__ __forceinline__ void sasa_centres(float *scen, const float *box, const float *qbox, const float *pc, int b, int Q)
{
    for (int j = threadIdx.x; j < Q; j += 256) {
        if (box) {
            scen[2 * j] = box[((size_t)b * Q + j) * 8];
            scen[2 * j + 1] = box[((size_t)b * Q + j) * 8 + 1];
        } else {
            const float *qb = qbox + ((size_t)b * Q + j) * 10;
            const float ang = qb[0] * SASA_TWO_PI, rad = qb[1] * 65.0f;
            const float xn = fminf(fmaxf((51.2f + rad * cosf(ang)) / 102.4f, 0.f), 1.f);
            const float yn = fminf(fmaxf((51.2f + rad * sinf(ang)) / 102.4f, 0.f), 1.f);
            scen[2 * j] = xn * (pc[3] - pc[0]) + pc[0];
            scen[2 * j + 1] = yn * (pc[4] - pc[1]) + pc[1];
        }
    }
}

// The attention mask (rac_sasa_fwd_mask / rac_sasa_bwd_mask).  A 16-key tile never straddles a 32-bit word, so what a lane needs
// of one mask row for one tile is a 16-bit field: bit k set = key tile*16 + k is blocked for that row.  The keys past Q are
// returned as blocked too (the padding bits of the operand are ignored), so a field of 0xffff means "no allowed key in this
// tile" and a tile whose 16 rows all say so is skipped by the whole wave: the decision comes from the mask words alone.
// Computing every tile instead gives the same results bit for bit: a blocked pair contributes an exact zero either way.

__device__ __forceinline__ unsigned sasa_mask_field(const unsigned *mask, int ld_mask, int row, int tile, int Q)
{
    const unsigned w = mask[(size_t)row * ld_mask + (tile >> 1)];
    const int nv = Q - tile * 16;   // keys of the tile that exist (>= 1)
    const unsigned pad = nv >= 16 ? 0u : (0xffffu << nv) & 0xffffu;
    return ((w >> ((tile & 1) * 16)) & 0xffffu) | pad;
}

// wave-uniform: no lane of the wave has an allowed pair in its field(s)
__device__ __forceinline__ bool sasa_all_blocked(unsigned field)
{
    return __builtin_amdgcn_ballot_w64(field != 0xffffu) == 0;
}

template <bool MASKED>
__global__ __launch_bounds__(256) void sasa_mfma_kernel(const SasaArgs a)
{
    extern __shared__ float smem[];
    float *scen = smem;                       // [Q][2] key centres (metres)
    float *sred = smem + 2 * ((a.Q + 1) & ~1);  // [4 waves][16] max, then [4][16] sum
    float *so = sred + 2 * 4 * 16;            // [4 waves][32 ch][16 queries]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    int bid = blockIdx.x;
    const int rb = bid % a.row_blocks; bid /= a.row_blocks;
    const int h = bid % a.H;
    const int b = bid / a.H;
    const int Q = a.Q, H = a.H;
    const size_t tok = (size_t)b * Q;
    const int ld = a.ld_qkv;

    sasa_centres(scen, a.box, a.qbox, a.pc, b, Q);
    // this lane's query column
    const int qi = rb * SASA_ROWS + li;
    const int qc = qi < Q ? qi : Q - 1;
    const float scale = 0.17677669529663687f;
    rac_f4 qb4[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        qb4[u] = rac_ld4(a.qkv + (tok + qc) * ld + h * SASA_D + 16 * u + 4 * lk);
        qb4[u].x *= scale; qb4[u].y *= scale; qb4[u].z *= scale; qb4[u].w *= scale;
    }
    const float tau = a.tau[(tok + qc) * a.ld_tau + h];
    __syncthreads();
    const float cqx = scen[2 * qc], cqy = scen[2 * qc + 1];

    const int ntiles = (Q + 15) >> 4;
    sasa_f4 sc[SASA_NT];
    float mloc = -INFINITY;
    // K rows one tile ahead of their MFMAs (two register sets; the loads of tile jt + 1 are pinned above the MFMAs of tile
    // jt): without this every tile waited out its own L2 latency -- 15 round trips per wave
    auto load_k = [&](int jt, rac_f4 &k0, rac_f4 &k1) {
        const int tile = wave + 4 * jt;
        const int key = tile * 16 + li;
        const int kc = key < Q ? key : Q - 1;
        const float *kp = a.qkv + (tok + kc) * ld + (H + h) * SASA_D + 4 * lk;
        k0 = rac_ld4(kp);
        k1 = rac_ld4(kp + 16);
    };
    // masked: this lane's 16-bit field of every tile of the wave (two to a register) and, wave-uniform, the tiles that are left
    // out: past the end, or without an allowed pair -- those load no K / V rows and issue no MFMAs
    unsigned mfield[MASKED ? SASA_NT / 2 : 1] = {};
    unsigned skip = 0;
    if constexpr (MASKED) {
#pragma unroll
        for (int jt = 0; jt < SASA_NT; ++jt) {
            const int tile = wave + 4 * jt;
            const unsigned f = tile < ntiles ? sasa_mask_field(a.mask, a.ld_mask, qc, tile, Q) : 0xffffu;
            mfield[jt >> 1] |= f << ((jt & 1) * 16);
            if (tile >= ntiles || sasa_all_blocked(f))
                skip |= 1u << jt;
        }
    }
    rac_f4 kb[2][2];
    if (!MASKED || !(skip & 1u))
        load_k(0, kb[0][0], kb[0][1]);
#pragma unroll
    for (int jt = 0; jt < SASA_NT; ++jt) {
        const int tile = wave + 4 * jt;
        sc[jt] = (sasa_f4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (jt + 1 < SASA_NT && (!MASKED || !((skip >> (jt + 1)) & 1u)))
            load_k(jt + 1, kb[(jt + 1) & 1][0], kb[(jt + 1) & 1][1]);     // (clamped to a valid row past the end)
        __builtin_amdgcn_sched_barrier(0);
        if (MASKED ? !((skip >> jt) & 1u) : tile < ntiles) {
            const rac_f4 k0 = kb[jt & 1][0], k1 = kb[jt & 1][1];
            sasa_f4 acc = {0.f, 0.f, 0.f, 0.f};
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k0.x, qb4[0].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k0.y, qb4[0].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k0.z, qb4[0].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k0.w, qb4[0].w, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k1.x, qb4[1].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k1.y, qb4[1].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k1.z, qb4[1].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(k1.w, qb4[1].w, acc, 0, 0, 0);
            // acc[r] = (q_query . k_key)/sqrt(d) for key = tile*16 + 4*lk + r, query = li; add the distance mask
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kk = tile * 16 + 4 * lk + r;
                bool allowed = kk < Q;
                if constexpr (MASKED)   // (the field has the keys past Q set)
                    allowed = !((mfield[jt >> 1] >> ((jt & 1) * 16 + 4 * lk + r)) & 1u);
                if (allowed) {
                    const float dx = cqx - scen[2 * kk], dy = cqy - scen[2 * kk + 1];
                    const float v = acc[r] - sqrtf(dx * dx + dy * dy) * tau;
                    sc[jt][r] = v;
                    mloc = fmaxf(mloc, v);
                }
            }
        }
    }
    // per-query max: over lk inside the wave, then over the four waves
    mloc = fmaxf(mloc, __shfl_xor(mloc, 16, 64));
    mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
    if (lk == 0)
        sred[wave * 16 + li] = mloc;
    __syncthreads();
    const float m = fmaxf(fmaxf(sred[li], sred[16 + li]), fmaxf(sred[32 + li], sred[48 + li]));
    float lsum = 0.f;
#pragma unroll
    for (int jt = 0; jt < SASA_NT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = (sc[jt][r] == -INFINITY) ? 0.f : expf(sc[jt][r] - m);
            sc[jt][r] = p;
            lsum += p;
        }
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    if (lk == 0)
        sred[64 + wave * 16 + li] = lsum;
    // O^T[ch][query] = sum_keys V[key][ch] * P^T[key][query]
    sasa_f4 oacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    // (V rows one tile ahead as well)
    auto load_v = [&](int jt, float (&va)[2][4]) {
        const int tile = wave + 4 * jt;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = tile * 16 + 4 * lk + i;
            const int kc = key < Q ? key : Q - 1;
            const float *vp = a.qkv + (tok + kc) * ld + (2 * H + h) * SASA_D;
            va[0][i] = vp[li];
            va[1][i] = vp[16 + li];
        }
    };
    float vb[2][2][4];
    if (!MASKED || !(skip & 1u))
        load_v(0, vb[0]);
#pragma unroll
    for (int jt = 0; jt < SASA_NT; ++jt) {
        const int tile = wave + 4 * jt;
        if (jt + 1 < SASA_NT && (!MASKED || !((skip >> (jt + 1)) & 1u)))
            load_v(jt + 1, vb[(jt + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        if (MASKED ? !((skip >> jt) & 1u) : tile < ntiles) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                oacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(vb[jt & 1][0][i], sc[jt][i], oacc[0], 0, 0, 0);
                oacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(vb[jt & 1][1][i], sc[jt][i], oacc[1], 0, 0, 0);
            }
        }
    }
    // combine the four waves: so[wave][ch][query]
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            so[(wave * 32 + 16 * c + 4 * lk + r) * 16 + li] = oacc[c][r];
    __syncthreads();
    {
        const int qq = tid >> 4, cp = (tid & 15) * 2;   // query within the tile, channel pair
        const int qrow = rb * SASA_ROWS + qq;
        if (qrow < Q) {
            const float l = (sred[64 + qq] + sred[64 + 16 + qq]) + (sred[64 + 32 + qq] + sred[64 + 48 + qq]);
            float o0 = 0.f, o1 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                o0 += so[(w * 32 + cp) * 16 + qq];
                o1 += so[(w * 32 + cp + 1) * 16 + qq];
            }
            *reinterpret_cast<float2 *>(a.out + (tok + qrow) * (size_t)(H * SASA_D) + h * SASA_D + cp) =
                make_float2(o0 / l, o1 / l);
            if (a.lse && cp == 0) {
                const float m = fmaxf(fmaxf(sred[qq], sred[16 + qq]), fmaxf(sred[32 + qq], sred[48 + qq]));
                a.lse[((size_t)b * H + h) * Q + qrow] = m + logf(l);
            }
        }
    }
}

__global__ __launch_bounds__(256) void sasa_stream_mask_kernel(const SasaArgs a);   // (below, beside the backward whose helpers it shares)

// the argument checks and the launch of rac_sasa_fwd_ex (masked = false) and rac_sasa_fwd_mask
static int sasa_fwd_launch(const char *fn, bool masked, const float *qkv, const float *tau, const float *query_bbox,
                           const float *box_table, float *out, float *lse, const uint32_t *mask_bits, int ld_mask, int ld_qkv,
                           int ld_tau, int B, int Q, int heads, int dim, const float *pc_range, void *stream)
{
    RAC_CHECK_ARG(dim == SASA_D, "%s: head dim %d (the kernel is built for %d)", fn, dim, SASA_D);
    RAC_CHECK_ARG(B >= 0 && Q >= 0 && heads >= 1 && ld_tau >= heads && ld_qkv >= 3 * heads * dim && ld_qkv % 4 == 0, "%s: bad sizes B=%d Q=%d heads=%d", fn, B, Q, heads);
    RAC_CHECK_ARG((size_t)Q * 2 * sizeof(float) <= 48 * 1024, "%s: Q=%d too large for the LDS centre table", fn, Q);
    RAC_CHECK_ARG(!masked || ld_mask >= (Q + 31) / 32, "%s: ld_mask=%d shorter than the %d words of a mask row (Q=%d)", fn, ld_mask, (Q + 31) / 32, Q);
    if (B == 0 || Q == 0)
        return 0;
    RAC_CHECK_ARG(qkv && tau && query_bbox && out && pc_range, "%s: null pointer", fn);
    RAC_CHECK_ARG(!masked || mask_bits, "%s: null pointer (mask_bits)", fn);
    SasaArgs a;
    a.qkv = qkv; a.tau = tau; a.qbox = query_bbox; a.box = box_table; a.out = out; a.lse = lse;
    for (int i = 0; i < 6; ++i)
        a.pc[i] = pc_range[i];
    a.B = B; a.Q = Q; a.H = heads; a.ld_tau = ld_tau; a.ld_qkv = ld_qkv;
    a.row_blocks = (Q + SASA_ROWS - 1) / SASA_ROWS;
    a.mask = masked ? mask_bits : nullptr; a.ld_mask = masked ? ld_mask : 0;
    const int nb = B * heads * a.row_blocks;
    const size_t cen = (size_t)2 * ((Q + 1) & ~1);
    const size_t lds_mfma = (cen + 2 * 4 * 16 + 4 * 32 * 16) * sizeof(float);
    if (masked) {
        // register-resident up to Q = 1024 (with an all-zero mask: rac_sasa_fwd_ex bit for bit), the streaming kernel above
        if (Q <= 4 * SASA_NT * 16)
            hipLaunchKernelGGL(sasa_mfma_kernel<true>, dim3(nb), dim3(256), lds_mfma, (hipStream_t)stream, a);
        else
            hipLaunchKernelGGL(sasa_stream_mask_kernel, dim3(nb), dim3(256), lds_mfma, (hipStream_t)stream, a);
    } else if (Q <= 4 * SASA_NT * 16) {
        hipLaunchKernelGGL(sasa_mfma_kernel<false>, dim3(nb), dim3(256), lds_mfma, (hipStream_t)stream, a);
    } else {
        const size_t lds = (cen + 2 * SASA_TILE * SASA_KS) * sizeof(float);
        hipLaunchKernelGGL(sasa_d32_kernel, dim3(nb), dim3(256), lds, (hipStream_t)stream, a);
    }
    return rac_launch_status(fn);
}

extern "C" int rac_sasa_fwd_ex(const float *qkv, const float *tau, const float *query_bbox, const float *box_table,
                               float *out, float *lse, int ld_qkv, int ld_tau, int B, int Q, int heads, int dim,
                               const float *pc_range, void *stream)
{
    return sasa_fwd_launch("rac_sasa_fwd_ex", false, qkv, tau, query_bbox, box_table, out, lse, nullptr, 0, ld_qkv, ld_tau, B, Q,
                           heads, dim, pc_range, stream);
}

extern "C" int rac_sasa_fwd_mask(const float *qkv, const float *tau, const float *query_bbox, const float *box_table,
                                 float *out, float *lse, int ld_qkv, int ld_tau, int B, int Q, int heads, int dim,
                                 const float *pc_range, void *stream, const uint32_t *mask_bits, int ld_mask)
{
    return sasa_fwd_launch("rac_sasa_fwd_mask", true, qkv, tau, query_bbox, box_table, out, lse, mask_bits, ld_mask, ld_qkv,
                           ld_tau, B, Q, heads, dim, pc_range, stream);
}

extern "C" int rac_sasa_fwd(const float *qkv, const float *tau, const float *query_bbox, const float *box_table,
                            float *out, int ld_qkv, int ld_tau, int B, int Q, int heads, int dim, const float *pc_range,
                            void *stream)
{
    return rac_sasa_fwd_ex(qkv, tau, query_bbox, box_table, out, nullptr, ld_qkv, ld_tau, B, Q, heads, dim, pc_range, stream);
}

// ---------------------------------------------------------------------------------------------------
// Backward.  With s_ij = (q_i . k_j)/sqrt(d) - r_ij tau_i, P = exp(s - lse), D_i = dO_i . O_i:
//   dP = dO V^T,  dS = P o (dP - D),  dq = dS K / sqrt(d),  dk = dS^T Q / sqrt(d),  dv = P^T dO,  dtau_i = -sum_j dS_ij r_ij.
// S is recomputed from the forward's lse: nothing of size Q x Q touches HBM.  One launch, two workgroup roles, each the
// forward's MFMA structure (v_mfma_f32_16x16x4_f32, exact fp32) streamed over all tiles of the other index, so every Q the
// forward accepts runs here (the statistics come in; no tile of S is kept across the loop):
//   row role    (blocks [0, n)):  16 queries of one (batch, head); the 4 waves take the 16-key tiles round-robin.
//     S^T and dP^T [16 keys x 16 queries] = K.Q^T and V.dO^T (A: key rows, B: the workgroup's query rows, as the forward), and
//     dS^T in the same accumulator layout is the B operand of dq^T [32 ch x 16 queries] = K^T . dS^T.  dtau is a register sum.
//   column role (blocks [n, 2n)): 16 keys of one (batch, head); the 4 waves take the 16-query tiles round-robin.
//     S and dP [16 queries x 16 keys] = Q.K^T and dO.V^T (A: query rows, B: the workgroup's key rows), so P and dS are the B
//     operands of dv^T [32 ch x 16 keys] = dO^T . P and dk^T = (Q/sqrt(d))^T . dS.
// Each role forms D_i itself from dO and O (a 32-wide dot, the same lanes and order in both), so the roles are independent.
// The four waves' partial sums are combined through LDS in a fixed order: every output element has one writer and no
// atomics, so the result is bit-reproducible.
struct SasaBwdArgs {
    const float *qkv, *tau, *qbox, *box, *out, *lse, *gout;
    float *gqkv, *gtau;
    float pc[6];
    int B, Q, H, ld_qkv, ld_tau, ld_gqkv, ld_gtau;
    int row_blocks;
    const unsigned *mask;  // masked instantiation only, as in SasaArgs
    int ld_mask;
};

#define SASA_MFMA8(acc, a4, b4)                                                       \
    do {                                                                              \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[0].x, b4[0].x, acc, 0, 0, 0);   \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[0].y, b4[0].y, acc, 0, 0, 0);   \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[0].z, b4[0].z, acc, 0, 0, 0);   \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[0].w, b4[0].w, acc, 0, 0, 0);   \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[1].x, b4[1].x, acc, 0, 0, 0);   \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[1].y, b4[1].y, acc, 0, 0, 0);   \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[1].z, b4[1].z, acc, 0, 0, 0);   \
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[1].w, b4[1].w, acc, 0, 0, 0);   \
    } while (0)

// channels 16u + 4*lk .. +3 (u = 0, 1) of a token row: the 8 k-steps of a 32-deep product as the forward assigns them
__device__ __forceinline__ void sasa_row8(rac_f4 (&v)[2], const float *row, int lk, float mul)
{
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        v[u] = rac_ld4(row + 16 * u + 4 * lk);
        v[u].x *= mul; v[u].y *= mul; v[u].z *= mul; v[u].w *= mul;
    }
}

__device__ __forceinline__ float sasa_dot8(const rac_f4 (&a)[2], const rac_f4 (&b)[2])
{
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u)
        s += a[u].x * b[u].x + a[u].y * b[u].y + a[u].z * b[u].z + a[u].w * b[u].w;
    return s;
}

// the four waves' [32 ch x 16] accumulators -> so[wave][ch][col]; after the barrier thread t sums column t>>4, channels
// 2(t&15), +1 over the waves in a fixed order
__device__ __forceinline__ float2 sasa_combine(float *so, const sasa_f4 (&acc)[2], int wave, int li, int lk)
{
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            so[(wave * 32 + 16 * c + 4 * lk + r) * 16 + li] = acc[c][r];
    __syncthreads();
    const int col = threadIdx.x >> 4, cp = (threadIdx.x & 15) * 2;
    float o0 = 0.f, o1 = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        o0 += so[(w * 32 + cp) * 16 + col];
        o1 += so[(w * 32 + cp + 1) * 16 + col];
    }
    return make_float2(o0, o1);
}

// ---------------------------------------------------------------------------------------------------
// Masked forward for Q > 1024 (rac_sasa_fwd_mask): the matrix-core forward as a stream over the key tiles, like the backward's
// row role -- one tile in flight per wave, nothing kept per tile, so every Q the centre table admits runs here.  Online softmax:
// a wave carries, per query column, the running max m and sum l of the tiles it has seen and the O^T accumulator scaled to m; a
// tile whose max raises m rescales l and the accumulator (eight multiplies a lane: the accumulator's query is the lane's own
// column li, so the factor needs no exchange).  The tile max goes over the four lk groups with two DPP steps.  One pass over K
// and V and 16 MFMAs a tile; the two-pass alternative (statistics first, then P V against the final max) forms every S tile
// twice -- 24 MFMAs and the K rows read twice -- to save the rescale, which is the cheaper of the two here.  The four waves'
// states are merged through LDS in a fixed order (log-sum-exp of the four maxima).  A tile without an allowed pair is skipped by
// the whole wave before any of its loads.  A query's result depends on its own allowed keys only: blocked pairs enter as exact zeros.
__global__ __launch_bounds__(256) void sasa_stream_mask_kernel(const SasaArgs a)
{
    extern __shared__ float smem[];
    float *scen = smem;                         // [Q][2] key centres (metres)
    float *sred = smem + 2 * ((a.Q + 1) & ~1);  // [4 waves][16] max, then [4][16] sum
    float *so = sred + 2 * 4 * 16;              // [4 waves][32 ch][16 queries]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    int bid = blockIdx.x;
    const int rb = bid % a.row_blocks; bid /= a.row_blocks;
    const int h = bid % a.H;
    const int b = bid / a.H;
    const int Q = a.Q, H = a.H;
    const size_t tok = (size_t)b * Q;
    const int ld = a.ld_qkv;
    const float scale = 0.17677669529663687f;

    sasa_centres(scen, a.box, a.qbox, a.pc, b, Q);
    const int qi = rb * SASA_ROWS + li;
    const int qc = qi < Q ? qi : Q - 1;
    rac_f4 qs[2];
    sasa_row8(qs, a.qkv + (tok + qc) * ld + h * SASA_D, lk, scale);
    const float tau = a.tau[(tok + qc) * a.ld_tau + h];
    __syncthreads();
    const float cqx = scen[2 * qc], cqy = scen[2 * qc + 1];

    const int ntiles = (Q + 15) >> 4;
    float m = -INFINITY, l = 0.f;   // m: the same in the four lanes of a query column; l: this lane's share of the sum
    sasa_f4 oacc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    for (int tile = wave; tile < ntiles; tile += 4) {
        const unsigned field = sasa_mask_field(a.mask, a.ld_mask, qc, tile, Q);
        if (sasa_all_blocked(field))
            continue;
        const int k0 = tile * 16;
        const int kr = k0 + li < Q ? k0 + li : Q - 1;
        rac_f4 kA[2];
        sasa_row8(kA, a.qkv + (tok + kr) * ld + (H + h) * SASA_D, lk, 1.f);
        // V^T operand of O^T: V[key k0 + 4lk + i][channel li (+16)]
        float vt[2][4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int key = k0 + 4 * lk + i;
            const float *vp = a.qkv + (tok + (key < Q ? key : Q - 1)) * ld + (2 * H + h) * SASA_D;
            vt[0][i] = vp[li];
            vt[1][i] = vp[16 + li];
        }
        sasa_f4 s = {0.f, 0.f, 0.f, 0.f};
        SASA_MFMA8(s, kA, qs);     // s[r] = S^T[key k0 + 4lk + r][query li]
        float tmax = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int kk = k0 + 4 * lk + r;
            const int kc = kk < Q ? kk : Q - 1;
            const float dx = cqx - scen[2 * kc], dy = cqy - scen[2 * kc + 1];
            const float v = s[r] - sqrtf(dx * dx + dy * dy) * tau;
            s[r] = ((field >> (4 * lk + r)) & 1u) ? -INFINITY : v;
            tmax = fmaxf(tmax, s[r]);
        }
        tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mn = fmaxf(m, tmax);   // (-inf only while the column has met no allowed key: then m is -inf too)
        const float corr = (m == -INFINITY) ? 0.f : expf(m - mn);
        l *= corr;
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                oacc[c][r] *= corr;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = (s[r] == -INFINITY) ? 0.f : expf(s[r] - mn);
            l += s[r];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            oacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(vt[0][i], s[i], oacc[0], 0, 0, 0);
            oacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(vt[1][i], s[i], oacc[1], 0, 0, 0);
        }
        m = mn;
    }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (lk == 0) {
        sred[wave * 16 + li] = m;
        sred[64 + wave * 16 + li] = l;
    }
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            so[(wave * 32 + 16 * c + 4 * lk + r) * 16 + li] = oacc[c][r];
    __syncthreads();
    {
        const int qq = tid >> 4, cp = (tid & 15) * 2;   // query within the tile, channel pair
        const int qrow = rb * SASA_ROWS + qq;
        if (qrow < Q) {
            const float mm = fmaxf(fmaxf(sred[qq], sred[16 + qq]), fmaxf(sred[32 + qq], sred[48 + qq]));
            float lsum = 0.f, o0 = 0.f, o1 = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float mw = sred[w * 16 + qq];
                const float f = (mw == -INFINITY) ? 0.f : expf(mw - mm);
                lsum += sred[64 + w * 16 + qq] * f;
                o0 += so[(w * 32 + cp) * 16 + qq] * f;
                o1 += so[(w * 32 + cp + 1) * 16 + qq] * f;
            }
            *reinterpret_cast<float2 *>(a.out + (tok + qrow) * (size_t)(H * SASA_D) + h * SASA_D + cp) =
                make_float2(o0 / lsum, o1 / lsum);
            if (a.lse && cp == 0)
                a.lse[((size_t)b * H + h) * Q + qrow] = mm + logf(lsum);
        }
    }
}

template <bool MASKED>
__global__ __launch_bounds__(256) void sasa_bwd_kernel(const SasaBwdArgs a)
{
    extern __shared__ float smem[];
    float *scen = smem;                         // [Q][2] centres (metres)
    float *sred = smem + 2 * ((a.Q + 1) & ~1);  // [4 waves][16] dtau partials
    float *so = sred + 4 * 16;                  // [4 waves][32 ch][16]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 15, lk = lane >> 4;
    const int nblk = a.B * a.H * a.row_blocks;
    const bool row_role = (int)blockIdx.x < nblk;
    int bid = row_role ? blockIdx.x : blockIdx.x - nblk;
    const int rb = bid % a.row_blocks; bid /= a.row_blocks;
    const int h = bid % a.H;
    const int b = bid / a.H;
    const int Q = a.Q, H = a.H;
    const size_t tok = (size_t)b * Q;
    const int ld = a.ld_qkv, ldo = H * SASA_D;
    const float scale = 0.17677669529663687f;
    const float *lse = a.lse + ((size_t)b * H + h) * Q;
    const int ntiles = (Q + 15) >> 4;

    sasa_centres(scen, a.box, a.qbox, a.pc, b, Q);
    // this lane's row of the workgroup's 16 (query in the row role, key in the column role)
    const int own = rb * SASA_ROWS + li;
    const int oc = own < Q ? own : Q - 1;
    __syncthreads();

    if (row_role) {
        rac_f4 qs[2], go[2], o4[2];
        sasa_row8(qs, a.qkv + (tok + oc) * ld + h * SASA_D, lk, scale);
        sasa_row8(go, a.gout + (tok + oc) * ldo + h * SASA_D, lk, 1.f);
        sasa_row8(o4, a.out + (tok + oc) * ldo + h * SASA_D, lk, 1.f);
        float Di = sasa_dot8(go, o4);
        Di += __shfl_xor(Di, 16, 64);
        Di += __shfl_xor(Di, 32, 64);
        const float tau = a.tau[(tok + oc) * a.ld_tau + h], lse_i = lse[oc];
        const float cqx = scen[2 * oc], cqy = scen[2 * oc + 1];
        sasa_f4 dq[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        float dtau = 0.f;
        for (int tile = wave; tile < ntiles; tile += 4) {
            unsigned field = 0;   // masked: this query's blocked keys of the tile (the keys past Q included)
            if constexpr (MASKED) {
                field = sasa_mask_field(a.mask, a.ld_mask, oc, tile, Q);
                if (sasa_all_blocked(field))
                    continue;
            }
            const int k0 = tile * 16;
            const int kr = k0 + li < Q ? k0 + li : Q - 1;
            rac_f4 kA[2], vA[2];
            sasa_row8(kA, a.qkv + (tok + kr) * ld + (H + h) * SASA_D, lk, 1.f);
            sasa_row8(vA, a.qkv + (tok + kr) * ld + (2 * H + h) * SASA_D, lk, 1.f);
            // K^T operand of dq: K[key k0 + 4lk + i][channel li (+16)]
            float kt[2][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int key = k0 + 4 * lk + i;
                const float *kp = a.qkv + (tok + (key < Q ? key : Q - 1)) * ld + (H + h) * SASA_D;
                kt[0][i] = kp[li];
                kt[1][i] = kp[16 + li];
            }
            sasa_f4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            SASA_MFMA8(s, kA, qs);     // s[r]  = S^T[key k0 + 4lk + r][query li]
            SASA_MFMA8(dp, vA, go);    // dp[r] = dP^T[same]
            sasa_f4 ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = k0 + 4 * lk + r;
                const int kc = key < Q ? key : Q - 1;
                const float dx = cqx - scen[2 * kc], dy = cqy - scen[2 * kc + 1];
                const float dist = sqrtf(dx * dx + dy * dy);
                bool allowed = key < Q;
                if constexpr (MASKED)
                    allowed = !((field >> (4 * lk + r)) & 1u);
                const float p = allowed ? expf(s[r] - dist * tau - lse_i) : 0.f;
                ds[r] = p * (dp[r] - Di);
                dtau -= ds[r] * dist;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dq[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(kt[0][i], ds[i], dq[0], 0, 0, 0);
                dq[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(kt[1][i], ds[i], dq[1], 0, 0, 0);
            }
        }
        dtau += __shfl_xor(dtau, 16, 64);
        dtau += __shfl_xor(dtau, 32, 64);
        if (lk == 0)
            sred[wave * 16 + li] = dtau;
        const float2 g = sasa_combine(so, dq, wave, li, lk);   // (its barrier also publishes sred)
        const int col = tid >> 4, cp = (tid & 15) * 2, qrow = rb * SASA_ROWS + col;
        if (qrow < Q) {
            *reinterpret_cast<float2 *>(a.gqkv + (tok + qrow) * a.ld_gqkv + h * SASA_D + cp) = make_float2(g.x * scale, g.y * scale);
            if (cp == 0)
                a.gtau[(tok + qrow) * a.ld_gtau + h] = (sred[col] + sred[16 + col]) + (sred[32 + col] + sred[48 + col]);
        }
    } else {
        rac_f4 kB[2], vB[2];
        sasa_row8(kB, a.qkv + (tok + oc) * ld + (H + h) * SASA_D, lk, 1.f);
        sasa_row8(vB, a.qkv + (tok + oc) * ld + (2 * H + h) * SASA_D, lk, 1.f);
        const float ckx = scen[2 * oc], cky = scen[2 * oc + 1];
        sasa_f4 dk[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        sasa_f4 dv[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        for (int tile = wave; tile < ntiles; tile += 4) {
            const int q0 = tile * 16;
            // masked: the fields of queries q0 + 4lk + i for the workgroup's key tile rb (bit li: this lane's key); a query
            // past Q counts as blocked
            unsigned fq[4] = {0, 0, 0, 0};
            if constexpr (MASKED) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int qi = q0 + 4 * lk + i;
                    fq[i] = qi < Q ? sasa_mask_field(a.mask, a.ld_mask, qi, rb, Q) : 0xffffu;
                }
                if (sasa_all_blocked(fq[0] & fq[1] & fq[2] & fq[3]))
                    continue;
            }
            const int qr = q0 + li < Q ? q0 + li : Q - 1;
            rac_f4 qA[2], gA[2], oA[2];
            sasa_row8(qA, a.qkv + (tok + qr) * ld + h * SASA_D, lk, scale);
            sasa_row8(gA, a.gout + (tok + qr) * ldo + h * SASA_D, lk, 1.f);
            sasa_row8(oA, a.out + (tok + qr) * ldo + h * SASA_D, lk, 1.f);
            // D of query q0 + li (as the row role forms it), then moved to the lanes that hold query q0 + 4lk + r
            float Dq = sasa_dot8(gA, oA);
            Dq += __shfl_xor(Dq, 16, 64);
            Dq += __shfl_xor(Dq, 32, 64);
            // Q^T and dO^T operands: row q0 + 4lk + i, channel li (+16)
            float qt[2][4], gt[2][4], tq[4], lq[4], cx[4], cy[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int qi = q0 + 4 * lk + i;
                const size_t t = tok + (qi < Q ? qi : Q - 1);
                const float *qp = a.qkv + t * ld + h * SASA_D;
                const float *gp = a.gout + t * ldo + h * SASA_D;
                qt[0][i] = qp[li] * scale; qt[1][i] = qp[16 + li] * scale;
                gt[0][i] = gp[li]; gt[1][i] = gp[16 + li];
                tq[i] = a.tau[t * a.ld_tau + h];
                lq[i] = lse[t - tok];
                cx[i] = scen[2 * (t - tok)]; cy[i] = scen[2 * (t - tok) + 1];
            }
            sasa_f4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
            SASA_MFMA8(s, qA, kB);     // s[r]  = S[query q0 + 4lk + r][key li]
            SASA_MFMA8(dp, gA, vB);    // dp[r] = dP[same]
            sasa_f4 p, ds;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float D = __shfl(Dq, 4 * lk + r, 64);
                const float dx = cx[r] - ckx, dy = cy[r] - cky;
                const float dist = sqrtf(dx * dx + dy * dy);
                bool allowed = q0 + 4 * lk + r < Q;
                if constexpr (MASKED)
                    allowed = !((fq[r] >> li) & 1u);
                p[r] = allowed ? expf(s[r] - dist * tq[r] - lq[r]) : 0.f;
                ds[r] = p[r] * (dp[r] - D);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dv[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(gt[0][i], p[i], dv[0], 0, 0, 0);
                dv[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(gt[1][i], p[i], dv[1], 0, 0, 0);
                dk[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(qt[0][i], ds[i], dk[0], 0, 0, 0);
                dk[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(qt[1][i], ds[i], dk[1], 0, 0, 0);
            }
        }
        const int col = tid >> 4, cp = (tid & 15) * 2, krow = rb * SASA_ROWS + col;
        float *gk = a.gqkv + (tok + krow) * a.ld_gqkv;
        const float2 gkv = sasa_combine(so, dk, wave, li, lk);
        if (krow < Q)
            *reinterpret_cast<float2 *>(gk + (H + h) * SASA_D + cp) = gkv;
        __syncthreads();   // so is reused
        const float2 gvv = sasa_combine(so, dv, wave, li, lk);
        if (krow < Q)
            *reinterpret_cast<float2 *>(gk + (2 * H + h) * SASA_D + cp) = gvv;
    }
}

// the argument checks and the launch of rac_sasa_bwd (masked = false) and rac_sasa_bwd_mask
static int sasa_bwd_launch(const char *fn, bool masked, const float *qkv, const float *tau, const float *query_bbox,
                           const float *box_table, const float *out, const float *lse, const float *grad_out, float *grad_qkv,
                           float *grad_tau, const uint32_t *mask_bits, int ld_mask, int ld_qkv, int ld_tau, int ld_grad_qkv,
                           int ld_grad_tau, int B, int Q, int heads, int dim, const float *pc_range, void *stream)
{
    RAC_CHECK_ARG(dim == SASA_D, "%s: head dim %d (the kernel is built for %d)", fn, dim, SASA_D);
    RAC_CHECK_ARG(B >= 0 && Q >= 0 && heads >= 1 && ld_tau >= heads && ld_qkv >= 3 * heads * dim && ld_qkv % 4 == 0 &&
                      ld_grad_qkv >= 3 * heads * dim && ld_grad_qkv % 2 == 0 && ld_grad_tau >= heads,
                  "%s: bad sizes B=%d Q=%d heads=%d ld_qkv=%d ld_tau=%d ld_grad_qkv=%d ld_grad_tau=%d", fn, B, Q, heads,
                  ld_qkv, ld_tau, ld_grad_qkv, ld_grad_tau);
    RAC_CHECK_ARG((size_t)Q * 2 * sizeof(float) <= 48 * 1024, "%s: Q=%d too large for the LDS centre table", fn, Q);
    RAC_CHECK_ARG(!masked || ld_mask >= (Q + 31) / 32, "%s: ld_mask=%d shorter than the %d words of a mask row (Q=%d)", fn, ld_mask, (Q + 31) / 32, Q);
    if (B == 0 || Q == 0)
        return 0;
    RAC_CHECK_ARG(qkv && tau && query_bbox && out && lse && grad_out && grad_qkv && grad_tau && pc_range,
                  "%s: null pointer", fn);
    RAC_CHECK_ARG(!masked || mask_bits, "%s: null pointer (mask_bits)", fn);
    SasaBwdArgs a;
    a.qkv = qkv; a.tau = tau; a.qbox = query_bbox; a.out = out; a.lse = lse; a.gout = grad_out;
    // the centres the forward used: the unmasked VALU kernel (Q > 1024) always decodes the boxes itself; both masked forwards
    // read the table when there is one
    a.box = (masked || Q <= 4 * SASA_NT * 16) ? box_table : nullptr;
    a.gqkv = grad_qkv; a.gtau = grad_tau;
    for (int i = 0; i < 6; ++i)
        a.pc[i] = pc_range[i];
    a.B = B; a.Q = Q; a.H = heads; a.ld_qkv = ld_qkv; a.ld_tau = ld_tau; a.ld_gqkv = ld_grad_qkv; a.ld_gtau = ld_grad_tau;
    a.row_blocks = (Q + SASA_ROWS - 1) / SASA_ROWS;
    a.mask = masked ? mask_bits : nullptr; a.ld_mask = masked ? ld_mask : 0;
    const int nb = 2 * B * heads * a.row_blocks;
    const size_t lds = ((size_t)2 * ((Q + 1) & ~1) + 4 * 16 + 4 * 32 * 16) * sizeof(float);
    if (masked)
        hipLaunchKernelGGL(sasa_bwd_kernel<true>, dim3(nb), dim3(256), lds, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(sasa_bwd_kernel<false>, dim3(nb), dim3(256), lds, (hipStream_t)stream, a);
    return rac_launch_status(fn);
}

extern "C" int rac_sasa_bwd(const float *qkv, const float *tau, const float *query_bbox, const float *box_table,
                            const float *out, const float *lse, const float *grad_out, float *grad_qkv, float *grad_tau,
                            int ld_qkv, int ld_tau, int ld_grad_qkv, int ld_grad_tau, int B, int Q, int heads, int dim,
                            const float *pc_range, void *stream)
{
    return sasa_bwd_launch("rac_sasa_bwd", false, qkv, tau, query_bbox, box_table, out, lse, grad_out, grad_qkv, grad_tau, nullptr,
                           0, ld_qkv, ld_tau, ld_grad_qkv, ld_grad_tau, B, Q, heads, dim, pc_range, stream);
}

extern "C" int rac_sasa_bwd_mask(const float *qkv, const float *tau, const float *query_bbox, const float *box_table,
                                 const float *out, const float *lse, const float *grad_out, float *grad_qkv, float *grad_tau,
                                 int ld_qkv, int ld_tau, int ld_grad_qkv, int ld_grad_tau, int B, int Q, int heads, int dim,
                                 const float *pc_range, void *stream, const uint32_t *mask_bits, int ld_mask)
{
    return sasa_bwd_launch("rac_sasa_bwd_mask", true, qkv, tau, query_bbox, box_table, out, lse, grad_out, grad_qkv, grad_tau,
                           mask_bits, ld_mask, ld_qkv, ld_tau, ld_grad_qkv, ld_grad_tau, B, Q, heads, dim, pc_range, stream);
}
