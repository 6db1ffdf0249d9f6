// frames.hip -- the streaming detector's window gather (gfx950): the decoder's inputs assembled from the frame memory.
//
// RaCFormer.simple_test_online (racformer_amd/detector.py) keeps the per-frame outputs of the front end -- the four pyramid levels in
// the sampling layout, the LSS BEV map and the radar BEV map -- in one ring of slots per tensor kind.  The decoder reads a window of T
// frames as T consecutive frames of one buffer per kind (buffers that stay put: the inputs of a captured step, racformer_amd/graph.py),
// so every step copies T frames of every kind from their slots to their places in the window:
//     outs[k][t * frame_bytes[k] ..] = rings[k][slots[t] * frame_bytes[k] ..]         k < n_tensors, t < T
// One launch for all kinds.  The tables (pointers, frame sizes, slots) travel as kernel arguments in one struct, as this library's
// descriptors do: no device table, no upload, nothing to synchronise with, nothing allocated.  16 bytes per lane on both sides; a
// workgroup moves pieces of 16 KB (256 lanes x 4 accesses, the four loads issued before the four stores), a tail piece inside a frame
// is cut lane by lane.  The workgroups are divided among the kinds in proportion to their bytes, so the 92 MB of pyramid frames and
// the 17 MB BEV frames of the f8 configuration finish together instead of the small kinds idling most of the grid.
#include "rac_common.h"

#define RAC_FRAMES_MAX_TENSORS 8
#define RAC_FRAMES_MAX_T 16
#define FRAMES_THREADS 256
#define FRAMES_UNROLL 4
#define FRAMES_PIECE (FRAMES_THREADS * FRAMES_UNROLL)      // 16-byte units a workgroup moves per pass
#define FRAMES_MAX_WGS 2048

struct frames_desc {
    const uint4 *ring[RAC_FRAMES_MAX_TENSORS];
    uint4 *out[RAC_FRAMES_MAX_TENSORS];
    long frame_units[RAC_FRAMES_MAX_TENSORS];          // 16-byte units per frame
    int pieces_per_frame[RAC_FRAMES_MAX_TENSORS];
    int wg_begin[RAC_FRAMES_MAX_TENSORS + 1];          // tensor k owns workgroups wg_begin[k] .. wg_begin[k + 1] - 1
    int slots[RAC_FRAMES_MAX_T];
    int n_tensors, T;
};

__global__ __launch_bounds__(FRAMES_THREADS) void frames_gather_kernel(const frames_desc d)
{
    const int wg = blockIdx.x;
    int k = 0;
#pragma unroll
    for (int i = 1; i < RAC_FRAMES_MAX_TENSORS; ++i)
        k += (i < d.n_tensors && wg >= d.wg_begin[i]) ? 1 : 0;
    const int nwg = d.wg_begin[k + 1] - d.wg_begin[k];
    const long units = d.frame_units[k];
    const int ppf = d.pieces_per_frame[k];
    const int pieces = ppf * d.T;
    for (int piece = wg - d.wg_begin[k]; piece < pieces; piece += nwg) {
        const int t = piece / ppf;
        const long u0 = (long)(piece - t * ppf) * FRAMES_PIECE + threadIdx.x;
        const uint4 *__restrict__ src = d.ring[k] + (long)d.slots[t] * units;
        uint4 *__restrict__ dst = d.out[k] + (long)t * units;
        uint4 v[FRAMES_UNROLL];
#pragma unroll
        for (int j = 0; j < FRAMES_UNROLL; ++j) {
            const long u = u0 + j * FRAMES_THREADS;
            if (u < units)
                v[j] = src[u];
        }
#pragma unroll
        for (int j = 0; j < FRAMES_UNROLL; ++j) {
            const long u = u0 + j * FRAMES_THREADS;
            if (u < units)
                dst[u] = v[j];
        }
    }
}

extern "C" int rac_frames_gather(int n_tensors, const void *const *rings, void *const *outs, const int64_t *frame_bytes,
                                 const int32_t *slots, int T, int n_slots, void *stream)
{
    RAC_CHECK_ARG(n_tensors >= 1 && n_tensors <= RAC_FRAMES_MAX_TENSORS, "rac_frames_gather: n_tensors=%d (1..%d)", n_tensors,
                  RAC_FRAMES_MAX_TENSORS);
    RAC_CHECK_ARG(T >= 1 && T <= RAC_FRAMES_MAX_T, "rac_frames_gather: T=%d (1..%d)", T, RAC_FRAMES_MAX_T);
    RAC_CHECK_ARG(n_slots >= 1, "rac_frames_gather: n_slots=%d", n_slots);
    RAC_CHECK_ARG(rings && outs && frame_bytes && slots, "rac_frames_gather: null pointer");
    frames_desc d = {};
    d.n_tensors = n_tensors;
    d.T = T;
    for (int t = 0; t < T; ++t) {
        RAC_CHECK_ARG(slots[t] >= 0 && slots[t] < n_slots, "rac_frames_gather: slots[%d]=%d outside [0, %d)", t, (int)slots[t], n_slots);
        d.slots[t] = slots[t];
    }
    double total = 0.0;
    long all_pieces = 0;
    for (int k = 0; k < n_tensors; ++k) {
        RAC_CHECK_ARG(rings[k] && outs[k], "rac_frames_gather: null pointer (tensor %d)", k);
        RAC_CHECK_ARG(frame_bytes[k] > 0 && frame_bytes[k] % 16 == 0, "rac_frames_gather: frame_bytes[%d]=%ld is not a positive multiple of 16",
                      k, (long)frame_bytes[k]);
        RAC_CHECK_ARG(((reinterpret_cast<uintptr_t>(rings[k]) | reinterpret_cast<uintptr_t>(outs[k])) & 15) == 0,
                      "rac_frames_gather: pointers must be 16-byte aligned (tensor %d)", k);
        const long units = (long)(frame_bytes[k] / 16);
        const long ppf = (units + FRAMES_PIECE - 1) / FRAMES_PIECE;
        RAC_CHECK_ARG(ppf * T < (1L << 30), "rac_frames_gather: frame_bytes[%d]=%ld is too large", k, (long)frame_bytes[k]);
        d.ring[k] = reinterpret_cast<const uint4 *>(rings[k]);
        d.out[k] = reinterpret_cast<uint4 *>(outs[k]);
        d.frame_units[k] = units;
        d.pieces_per_frame[k] = (int)ppf;
        total += (double)frame_bytes[k];
        all_pieces += ppf * T;
    }
    // workgroups in proportion to the bytes, at least one per tensor and never more than a tensor has pieces
    const long budget = all_pieces < FRAMES_MAX_WGS ? all_pieces : FRAMES_MAX_WGS;
    int next = 0;
    for (int k = 0; k < n_tensors; ++k) {
        const long pieces = (long)d.pieces_per_frame[k] * T;
        long n = (long)((double)budget * ((double)frame_bytes[k] / total));
        n = n < 1 ? 1 : n;
        n = n > pieces ? pieces : n;
        d.wg_begin[k] = next;
        next += (int)n;
    }
    for (int k = n_tensors; k <= RAC_FRAMES_MAX_TENSORS; ++k)
        d.wg_begin[k] = next;
    hipLaunchKernelGGL(frames_gather_kernel, dim3((unsigned)next), dim3(FRAMES_THREADS), 0, (hipStream_t)stream, d);
    return rac_launch_status("rac_frames_gather");
}
