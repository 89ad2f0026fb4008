// kitti_anno.hip -- KITTI result annotations inside the captured frame (include/sassd.h "KITTI annotations"): the
// detection rows sassd_rescore_nms left behind -> camera-frame boxes, alpha and clipped 2-D boxes of the rows whose
// projection meets the image, compacted in detection (score) order.  The per-box arithmetic is box_anno of
// kitti_anno_core.h, the function the CPU harness of the tests evaluates.
//
// One workgroup of 256 threads per sample walks the capD rows in chunks of 256; the trip count comes from capD, so every
// thread reaches every barrier whatever counts[b] holds.  Rank of a kept row = rows kept in earlier chunks (a running
// base every thread carries) + rows kept by the lower waves of this chunk (4 LDS words) + kept lanes below it in its wave
// (ballot + mbcnt).  Rows at or past kept[b] are then written as zero words.  Plain loads and vector stores only.
#include "common.h"
#include "kitti_anno_core.h"

namespace {
using namespace sassd_kitti;

constexpr int kThreads = 256, kWaves = kThreads / SASSD_WAVE;

// the annotation block, in 32-bit words from its (8-byte aligned) start; n = B * capD
struct AnnoLayout {
    size_t kept, index, cam, alpha, pad, bbox, total_bytes;
};

inline AnnoLayout anno_layout(int B, int capD)
{
    const size_t n = (size_t)B * capD;
    AnnoLayout L;
    L.kept = 0;
    L.index = ((size_t)B + 1) / 2 * 2;          // kept[B], then a zero word when B is odd
    L.cam = L.index + n;
    L.alpha = L.cam + 7 * n;
    L.pad = L.alpha + n;                        // one zero word when n is odd: bbox starts on 8 bytes
    L.bbox = L.pad + (n & 1);
    L.total_bytes = 4 * L.bbox + 32 * n;
    return L;
}

struct AnnoParams {
    const float *boxes;
    const int32_t *counts;
    const double *calib;
    int32_t *out;
    AnnoLayout L;
    int B, capD;
};

__device__ __forceinline__ int lanes_below(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
}

__global__ void __launch_bounds__(kThreads) frame_annos_kernel(AnnoParams P)
{
    __shared__ int s_cnt[kWaves];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = P.counts[b];
    const int count = c < 0 ? 0 : (c > P.capD ? P.capD : c);            // seal_count of heads.hip
    const double *calib = P.calib + (size_t)b * kCalibDoubles;
    const size_t row0 = (size_t)b * P.capD;
    int32_t *o_index = P.out + P.L.index + row0;
    float *o_cam = (float *)(P.out + P.L.cam) + 7 * row0;
    float *o_alpha = (float *)(P.out + P.L.alpha) + row0;
    double *o_bbox = (double *)(P.out + P.L.bbox) + 4 * row0;

    int base = 0;                                                       // rows kept by the chunks before this one
    const int chunks = (P.capD + kThreads - 1) / kThreads;
    for (int ch = 0; ch < chunks; ++ch) {
        const int row = ch * kThreads + threadIdx.x;
        Anno a;
        a.keep = false;
        if (row < count) a = box_anno(P.boxes + (row0 + row) * 7, calib);
        const unsigned long long mask = __ballot(a.keep);
        if (lane == 0) s_cnt[wave] = __popcll(mask);
        __syncthreads();
        int mine = base;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) mine += s_cnt[w];
            base += s_cnt[w];
        }
        if (a.keep) {
            const int r = mine + lanes_below(mask);                     // r <= row < capD
            o_index[r] = row;
#pragma unroll
            for (int k = 0; k < 7; ++k) o_cam[7 * (size_t)r + k] = a.cam[k];
            o_alpha[r] = a.alpha;
#pragma unroll
            for (int k = 0; k < 4; ++k) o_bbox[4 * (size_t)r + k] = a.bbox[k];
        }
        __syncthreads();                                                // s_cnt is rewritten by the next chunk
    }
    for (int r = base + threadIdx.x; r < P.capD; r += kThreads) {       // base == kept[b]
        o_index[r] = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) o_cam[7 * (size_t)r + k] = 0.f;
        o_alpha[r] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) o_bbox[4 * (size_t)r + k] = 0.0;
    }
    if (threadIdx.x == 0) {
        P.out[P.L.kept + b] = base;
        if (b == 0) {                                                   // the two padding words of the block
            if (P.B & 1) P.out[P.L.kept + P.B] = 0;
            if (P.L.bbox != P.L.pad) P.out[P.L.pad] = 0;
        }
    }
}
}  // namespace

extern "C" size_t sassd_frame_annos_bytes(int batch, int capD)
{
    if (batch < 1 || capD < 1 || (long)batch * capD > (1L << 24)) return 0;
    return anno_layout(batch, capD).total_bytes;
}

extern "C" int sassd_frame_annos(const float *boxes, const int32_t *counts, int batch, int capD, const double *calib,
                                 void *annos, size_t annos_bytes, void *stream_)
{
    if (!boxes || !counts || !calib || !annos) return SASSD_EINVAL;
    const size_t need = sassd_frame_annos_bytes(batch, capD);
    if (need == 0) return SASSD_EINVAL;
    if (((uintptr_t)boxes & 3) || ((uintptr_t)counts & 3) || ((uintptr_t)calib & 7) || ((uintptr_t)annos & 7))
        return SASSD_EINVAL;
    if (annos_bytes < need) return SASSD_ENOSPC;
    AnnoParams P;
    P.boxes = boxes; P.counts = counts; P.calib = calib; P.out = (int32_t *)annos;
    P.L = anno_layout(batch, capD); P.B = batch; P.capD = capD;
    hipLaunchKernelGGL(frame_annos_kernel, dim3(batch), dim3(kThreads), 0, (hipStream_t)stream_, P);
    return sassd_launch_status();
}
