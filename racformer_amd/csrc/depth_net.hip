// depth_net.hip -- DepthNet of LSSViewTransformerBEVDepth_racformer (models/necks/view_transformer_racformer.py:329-567 of the
// reference, use_dcn=False) in eval mode with every BatchNorm folded into its neighbour: a convolution for many small maps and
// the per-image vectors around it, gfx950.
//
//   cs_pack_kernel       channel-first [BN, C, hw] -> channel-last rows at a channel offset (a 32 x 32 transpose through LDS),
//                        zero padding behind them
//   cs_conv_kernel       1x1 or 3x3 (any dilation, padding = dilation) over channel-last rows as an implicit GEMM on the exact-fp32
//                        MFMA: one workgroup = 64 pixels of ONE image x 64 output channels, four waves of one 32 x 32 tile each;
//                        K runs over (live tap, 32 input channels), the next step's operands are in flight while this one's 16
//                        MFMAs issue.  A 16 x 44 map is 11 tiles, so six maps x 256 channels are 264 workgroups -- the 256-pixel
//                        x 256-channel tile of conv3x3.hip makes 18.  Taps that cannot hit the image are never staged.
//                        Prologue: a per-image gate on the input channels.  Epilogue, in this order: + bias, + per-image bias,
//                        + one table row per pixel picked by an int32 map (twice: depth bin, RCS class), + residual, ReLU;
//                        to channel-last rows at a channel offset (the next layer's operand, so a concatenation is never
//                        copied) or channel-first.
//   dn_gates_kernel      mlp_input row -> Mlp -> SE tail -> sigmoid: one workgroup per (image, branch)
//   dn_pool_bias_kernel  mean over a map's pixels -> 1x1 + ReLU -> the image-pool branch's share of ASPP.conv1 as a per-image bias
//
// v_mfma_f32_32x32x2_f32 is an fmaf chain in K order, bit for bit: no operand is rounded below fp32 and no activation scale is
// needed.  The chain restarts every 32 input channels and the partial sums are added in fp32.  Every sum has one fixed order,
// nothing is atomic and nothing is read back: capturable, bitwise reproducible.
#include "rac_common.h"

#define CS_TM 64        // pixels of a workgroup
#define CS_TN 64        // output channels of a workgroup
#define CS_TK 32        // input channels of a K step
#define CS_LDA 66       // As[k][pixel]: a thread stores channels 4q..4q+3 of pixel p at banks 8q + p + const (q, p < 8): distinct
#define CS_LDB 68       // Bs[k][channel]: rows stay 16-byte aligned
#define DN_MAX_C 1024

typedef float cs_f16v __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void cs_pack_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int hw, int ld_dst,
                                                      int c_off, int c_total)
{
    __shared__ float tile[32][33];
    const int n = blockIdx.z, p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 8 rows of 32 lanes
    for (int j = ty; j < 32; j += 8) {
        const int c = c0 + j, p = p0 + tx;
        tile[j][tx] = (c < C && p < hw) ? src[((size_t)n * C + c) * hw + p] : 0.f;
    }
    __syncthreads();
    for (int j = ty; j < 32; j += 8) {
        const int p = p0 + j, c = c0 + tx;
        if (p < hw && c < c_total)
            dst[((size_t)n * hw + p) * ld_dst + c_off + c] = tile[tx][j];
    }
}

__global__ __launch_bounds__(256) void cs_conv_kernel(const rac_conv_small d, int tiles_per_img)
{
    __shared__ __attribute__((aligned(16))) float As[CS_TK * CS_LDA];
    __shared__ __attribute__((aligned(16))) float Bs[CS_TK * CS_LDB];
    __shared__ int s_tap[9];
    __shared__ int s_ntap;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int n = blockIdx.x / tiles_per_img, p0 = (blockIdx.x % tiles_per_img) * CS_TM;
    const int co0 = blockIdx.y * CS_TN;
    const int H = d.H, W = d.W, hw = H * W, dil = d.dilation;

    if (t == 0) {
        int k = 0;
        if (d.ksize == 3) {
            for (int tp = 0; tp < 9; ++tp) {
                const int dy = (tp / 3 - 1) * dil, dx = (tp % 3 - 1) * dil;
                if (abs(dy) < H && abs(dx) < W)
                    s_tap[k++] = tp;
            }
        } else {
            s_tap[k++] = 0;
        }
        s_ntap = k;
    }
    __syncthreads();

    // staging roles.  A: pixels ap and ap + 32 of the tile, channels 4 aq .. 4 aq + 3 of the K step.  B: rows bk and bk + 16.
    const int ap = t >> 3, aq = t & 7;
    const int bk = t >> 4, bq = t & 15;
    int ph[2], pw[2];
    bool pv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int p = p0 + ap + 32 * j;
        pv[j] = p < hw;
        ph[j] = p / W;
        pw[j] = p % W;
    }
    const int chunks = d.Cin / CS_TK;
    const int steps = s_ntap * chunks;
    const float *in_n = d.in + (size_t)n * hw * d.ld_in;

    // The loads of step it + 1 are issued before step it's MFMAs and first touched when they are stored to LDS: every load is
    // unconditional (a tap outside the map reads a clamped, in-bounds address and is zeroed by a select at the store), and the
    // gate is multiplied in at the store too, so that nothing waits on memory between the barrier and the MFMAs.
    rac_f4 ra[2], rb[2], rg = {1.f, 1.f, 1.f, 1.f};
    bool rv[2], gated = false;
    auto fetch = [&](int it) {
        const int tp = s_tap[it / chunks], c0 = (it % chunks) * CS_TK;
        const int dy = d.ksize == 3 ? (tp / 3 - 1) * dil : 0, dx = d.ksize == 3 ? (tp % 3 - 1) * dil : 0;
        if (d.gate) {
            rg = rac_ld4(d.gate + (size_t)n * d.gate_channels + (c0 < d.gate_channels ? c0 : 0) + 4 * aq);
            gated = c0 < d.gate_channels;
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int sh = ph[j] + dy, sw = pw[j] + dx;
            rv[j] = pv[j] && sh >= 0 && sh < H && sw >= 0 && sw < W;
            const int ch = min(max(sh, 0), H - 1), cw = min(max(sw, 0), W - 1);
            ra[j] = rac_ld4(in_n + ((size_t)ch * W + cw) * d.ld_in + c0 + 4 * aq);
            rb[j] = rac_ld4(d.w + ((size_t)tp * d.Cin + c0 + bk + 16 * j) * d.ld_w + co0 + 4 * bq);
        }
    };

    cs_f16v zero;
#pragma unroll
    for (int r = 0; r < 16; ++r)
        zero[r] = 0.f;
    cs_f16v acc = zero;
    const int wm = wave & 1, wn = wave >> 1;
    const float *a_rd = As + (lane >> 5) * CS_LDA + wm * 32 + (lane & 31);
    const float *b_rd = Bs + (lane >> 5) * CS_LDB + wn * 32 + (lane & 31);

    fetch(0);
    for (int it = 0; it < steps; ++it) {
        const rac_f4 g = {gated ? rg.x : 1.f, gated ? rg.y : 1.f, gated ? rg.z : 1.f, gated ? rg.w : 1.f};
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float *a = As + (4 * aq) * CS_LDA + ap + 32 * j;
            a[0] = rv[j] ? ra[j].x * g.x : 0.f;
            a[CS_LDA] = rv[j] ? ra[j].y * g.y : 0.f;
            a[2 * CS_LDA] = rv[j] ? ra[j].z * g.z : 0.f;
            a[3 * CS_LDA] = rv[j] ? ra[j].w * g.w : 0.f;
            *reinterpret_cast<rac_f4 *>(Bs + (bk + 16 * j) * CS_LDB + 4 * bq) = rb[j];
        }
        __syncthreads();
        if (it + 1 < steps)
            fetch(it + 1);
        // blocked summation: the 32 products of a K step are chained inside the MFMA from zero, the steps are added in fp32 --
        // a 2304-term fmaf chain measured 4.8 x the float32 restatement's own error on the f8 map, above the project's 4 x rule
        cs_f16v part = zero;
#pragma unroll
        for (int kk = 0; kk < CS_TK / 2; ++kk)
            part = __builtin_amdgcn_mfma_f32_32x32x2f32(a_rd[2 * kk * CS_LDA], b_rd[2 * kk * CS_LDB], part, 0, 0, 0);
        acc += part;
        __syncthreads();
    }

    // lane: output channel co0 + 32 wn + (lane & 31); register r: pixel row 8 (r >> 2) + 4 (lane >> 5) + (r & 3) of the wave's 32
    const int co = co0 + wn * 32 + (lane & 31);
    if (co >= d.Cout)
        return;
    const float b0 = d.bias ? d.bias[co] : 0.f;
    const float b1 = d.img_bias ? d.img_bias[(size_t)n * d.Cout + co] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int p = p0 + wm * 32 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        if (p >= hw)
            continue;
        const size_t pix = (size_t)n * hw + p;
        float v = acc[r] + b0;
        if (d.img_bias)
            v += b1;
        if (d.bins) {
            const int b = d.bins[pix];
            if (b >= 0 && b < d.n_bins)
                v += d.bins_table[(size_t)b * d.Cout + co];
        }
        if (d.cls) {
            const int c = d.cls[pix];
            v += d.cls_table[(size_t)((c >= 0 && c < d.n_cls) ? c + 1 : 0) * d.Cout + co];
        }
        if (d.residual)
            v += d.residual[pix * d.ld_res + co];
        if (d.relu)
            v = rac_relu(v);
        if (d.out_layout == RAC_CS_CHANNEL_FIRST)
            d.out[((size_t)n * d.ld_out + d.c_off + co) * hw + p] = v;
        else
            d.out[pix * d.ld_out + d.c_off + co] = v;
    }
}

// params of one branch: w1t [9][C] | b1 [C] | w2t [C][C] | b2 [C] | wrt [C][C] | br [C] | wet [C][C] | be [C], all [in][out].
__global__ __launch_bounds__(256) void dn_gates_kernel(const float *__restrict__ mlp_input, const float *__restrict__ params,
                                                       float *__restrict__ gates, int BN, int C)
{
    __shared__ float u[DN_MAX_C], v[DN_MAX_C];
    __shared__ float x[9];
    const int n = blockIdx.x, br = blockIdx.y;
    const float *w1 = params + (size_t)br * (10 * (size_t)C + 3 * ((size_t)C * C + C));
    const float *b1 = w1 + 9 * C, *w2 = b1 + C, *b2 = w2 + (size_t)C * C, *wr = b2 + C, *brd = wr + (size_t)C * C, *we = brd + C,
                *be = we + (size_t)C * C;
    if (threadIdx.x < 9)
        x[threadIdx.x] = mlp_input[(size_t)n * 9 + threadIdx.x];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = b1[c];
        for (int k = 0; k < 9; ++k)
            s = fmaf(w1[k * C + c], x[k], s);
        u[c] = rac_relu(s);
    }
    __syncthreads();
    auto layer = [&](const float *w, const float *b, const float *src, float *dst, int act) {
        for (int c = threadIdx.x; c < C; c += 256) {
            float s = b[c];
#pragma unroll 8
            for (int k = 0; k < C; ++k)
                s = fmaf(w[(size_t)k * C + c], src[k], s);
            dst[c] = act == 1 ? rac_relu(s) : s;
        }
        __syncthreads();
    };
    layer(w2, b2, u, v, 0);
    layer(wr, brd, v, u, 1);
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = be[c];
#pragma unroll 8
        for (int k = 0; k < C; ++k)
            s = fmaf(we[(size_t)k * C + c], u[k], s);
        gates[((size_t)br * BN + n) * C + c] = 1.f / (1.f + expf(-s));
    }
}

// One workgroup of 1024 threads per image: G = 1024 / C pixel segments x C channels.  Segment g sums its pixels in ascending
// order, the segments are added in ascending order; mean = sum / hw.
__global__ __launch_bounds__(1024) void dn_pool_bias_kernel(const float *__restrict__ x, int ld, const float *__restrict__ wpool_t,
                                                            const float *__restrict__ bpool, const float *__restrict__ wbias_t,
                                                            float *__restrict__ img_bias, int hw, int C, int Cout)
{
    __shared__ float part[1024];
    __shared__ float m[DN_MAX_C], y[DN_MAX_C];
    const int n = blockIdx.x, G = 1024 / C;
    const int g = threadIdx.x / C, c = threadIdx.x % C;
    if (g < G) {
        const int q0 = (int)((long)hw * g / G), q1 = (int)((long)hw * (g + 1) / G);
        const float *px = x + (size_t)n * hw * ld + c;
        float s = 0.f;
#pragma unroll 8
        for (int q = q0; q < q1; ++q)
            s += px[(size_t)q * ld];
        part[g * C + c] = s;
    }
    __syncthreads();
    for (int cc = threadIdx.x; cc < C; cc += 1024) {
        float s = part[cc];
        for (int gg = 1; gg < G; ++gg)
            s += part[gg * C + cc];
        m[cc] = s / (float)hw;
    }
    __syncthreads();
    for (int cc = threadIdx.x; cc < C; cc += 1024) {
        float s = bpool[cc];
#pragma unroll 8
        for (int k = 0; k < C; ++k)
            s = fmaf(wpool_t[(size_t)k * C + cc], m[k], s);
        y[cc] = rac_relu(s);
    }
    __syncthreads();
    for (int co = threadIdx.x; co < Cout; co += 1024) {
        float s = 0.f;
#pragma unroll 8
        for (int k = 0; k < C; ++k)
            s = fmaf(wbias_t[(size_t)k * Cout + co], y[k], s);
        img_bias[(size_t)n * Cout + co] = s;
    }
}

static bool cs_aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int rac_conv_small_pack_fwd(const float *src, float *dst, int BN, int C, int hw, int ld_dst, int c_off, int c_pad,
                                       void *stream)
{
    RAC_CHECK_ARG(BN >= 0 && C >= 1 && hw >= 1 && c_off >= 0 && c_pad >= 0, "rac_conv_small_pack_fwd: BN=%d C=%d hw=%d c_off=%d c_pad=%d", BN,
                  C, hw, c_off, c_pad);
    RAC_CHECK_ARG((int64_t)c_off + C + c_pad <= ld_dst, "rac_conv_small_pack_fwd: channels %d..%d do not fit rows of %d", c_off,
                  c_off + C + c_pad, ld_dst);
    RAC_CHECK_ARG((int64_t)BN * hw * ld_dst < ((int64_t)1 << 31) && (int64_t)BN * hw * C < ((int64_t)1 << 31) && BN < 65536,
                  "rac_conv_small_pack_fwd: tensor too large");
    RAC_CHECK_ARG(src && dst, "rac_conv_small_pack_fwd: null pointer");
    if (BN == 0)
        return 0;
    hipLaunchKernelGGL(cs_pack_kernel, dim3((hw + 31) / 32, (C + c_pad + 31) / 32, BN), dim3(256), 0, (hipStream_t)stream, src, dst, C, hw,
                       ld_dst, c_off, C + c_pad);
    return rac_launch_status("rac_conv_small_pack_fwd");
}

extern "C" int rac_conv_small_fwd(const rac_conv_small *d, void *stream)
{
    RAC_CHECK_ARG(d, "rac_conv_small_fwd: null descriptor");
    RAC_CHECK_ARG(d->in && d->w && d->out, "rac_conv_small_fwd: null pointer (in, w or out)");
    RAC_CHECK_ARG(d->BN >= 0 && d->H >= 1 && d->W >= 1, "rac_conv_small_fwd: BN=%d H=%d W=%d", d->BN, d->H, d->W);
    RAC_CHECK_ARG(d->ksize == 1 || d->ksize == 3, "rac_conv_small_fwd: ksize=%d (1 or 3)", d->ksize);
    RAC_CHECK_ARG(d->dilation >= 1, "rac_conv_small_fwd: dilation=%d < 1", d->dilation);
    RAC_CHECK_ARG(d->Cin >= CS_TK && d->Cin % CS_TK == 0 && d->Cin <= 4096, "rac_conv_small_fwd: Cin=%d is not a multiple of %d in %d..4096",
                  d->Cin, CS_TK, CS_TK);
    RAC_CHECK_ARG(d->ld_in >= d->Cin && d->ld_in % 4 == 0 && cs_aligned16(d->in), "rac_conv_small_fwd: input rows of %d floats (>= Cin, 16-byte aligned)",
                  d->ld_in);
    RAC_CHECK_ARG(d->Cout >= 1 && d->ld_w >= d->Cout && d->ld_w % CS_TN == 0 && cs_aligned16(d->w),
                  "rac_conv_small_fwd: Cout=%d, weight rows of %d floats (a multiple of %d >= Cout, 16-byte aligned)", d->Cout, d->ld_w, CS_TN);
    RAC_CHECK_ARG(!d->gate || (d->gate_channels >= CS_TK && d->gate_channels % CS_TK == 0 && d->gate_channels <= d->Cin && cs_aligned16(d->gate)),
                  "rac_conv_small_fwd: gate_channels=%d is not a multiple of %d up to Cin", d->gate_channels, CS_TK);
    RAC_CHECK_ARG(!d->residual || d->ld_res >= d->Cout, "rac_conv_small_fwd: residual rows of %d floats < Cout", d->ld_res);
    RAC_CHECK_ARG(!d->bins || (d->bins_table && d->n_bins >= 1), "rac_conv_small_fwd: bins without a table");
    RAC_CHECK_ARG(!d->cls || (d->cls_table && d->n_cls >= 0), "rac_conv_small_fwd: cls without a table");
    RAC_CHECK_ARG(d->out_layout == RAC_CS_CHANNEL_LAST || d->out_layout == RAC_CS_CHANNEL_FIRST, "rac_conv_small_fwd: out_layout=%d",
                  d->out_layout);
    RAC_CHECK_ARG(d->c_off >= 0 && (int64_t)d->c_off + d->Cout <= d->ld_out, "rac_conv_small_fwd: channels %d..%d do not fit %d", d->c_off,
                  d->c_off + d->Cout, d->ld_out);
    const int64_t hw = (int64_t)d->H * d->W;
    RAC_CHECK_ARG(hw < ((int64_t)1 << 24) && d->BN * hw * d->ld_in < ((int64_t)1 << 31) && d->BN * hw * d->ld_out < ((int64_t)1 << 31),
                  "rac_conv_small_fwd: tensor too large");
    if (d->BN == 0)
        return 0;
    const int tiles = (int)((hw + CS_TM - 1) / CS_TM);
    RAC_CHECK_ARG((int64_t)tiles * d->BN < ((int64_t)1 << 31), "rac_conv_small_fwd: too many tiles");
    hipLaunchKernelGGL(cs_conv_kernel, dim3((unsigned)(tiles * d->BN), (d->Cout + CS_TN - 1) / CS_TN), dim3(256), 0, (hipStream_t)stream, *d,
                       tiles);
    return rac_launch_status("rac_conv_small_fwd");
}

extern "C" int rac_depthnet_gates_fwd(const float *mlp_input, const float *params, float *gates, int BN, int C, int branches, void *stream)
{
    RAC_CHECK_ARG(BN >= 0 && branches >= 1 && branches <= 64, "rac_depthnet_gates_fwd: BN=%d branches=%d", BN, branches);
    RAC_CHECK_ARG(C >= 1 && C <= DN_MAX_C, "rac_depthnet_gates_fwd: C=%d (1..%d)", C, DN_MAX_C);
    RAC_CHECK_ARG(mlp_input && params && gates, "rac_depthnet_gates_fwd: null pointer");
    if (BN == 0)
        return 0;
    hipLaunchKernelGGL(dn_gates_kernel, dim3(BN, branches), dim3(256), 0, (hipStream_t)stream, mlp_input, params, gates, BN, C);
    return rac_launch_status("rac_depthnet_gates_fwd");
}

extern "C" int rac_depthnet_pool_bias_fwd(const float *x, const float *wpool_t, const float *bpool, const float *wbias_t, float *img_bias,
                                          int BN, int hw, int ld, int C, int Cout, void *stream)
{
    RAC_CHECK_ARG(BN >= 0 && hw >= 1, "rac_depthnet_pool_bias_fwd: BN=%d hw=%d", BN, hw);
    RAC_CHECK_ARG(C >= 1 && C <= DN_MAX_C && ld >= C && Cout >= 1, "rac_depthnet_pool_bias_fwd: C=%d (1..%d) ld=%d Cout=%d", C, DN_MAX_C, ld,
                  Cout);
    RAC_CHECK_ARG((int64_t)BN * hw * ld < ((int64_t)1 << 31), "rac_depthnet_pool_bias_fwd: tensor too large");
    RAC_CHECK_ARG(x && wpool_t && bpool && wbias_t && img_bias, "rac_depthnet_pool_bias_fwd: null pointer");
    if (BN == 0)
        return 0;
    hipLaunchKernelGGL(dn_pool_bias_kernel, dim3(BN), dim3(1024), 0, (hipStream_t)stream, x, ld, wpool_t, bpool, wbias_t, img_bias, hw, C,
                       Cout);
    return rac_launch_status("rac_depthnet_pool_bias_fwd");
}
