// box_fuse.hip -- box fusion behind rescore + NMS (include/sassd.h "Box fusion"): every detection becomes the score-weighted
// mean of the candidates of its label that overlap it, itself included, instead of the one box that survived.
//
//   box_fuse_kernel    ONE WAVE per detection, kWaves waves per workgroup, grid (ceil(capD / kWaves), batch).  Two steps, because
//                      the rotated IoU is some thousand instructions and a lane that needs it holds up its whole wave:
//                      (1) SCREEN.  The lanes stride the sample's candidates in chunks of 64: score (sigmoidf of sigmoid.h, as
//                          rescore_prep_kernel), label, and a circumscribed-circle test that only drops pairs whose overlap is
//                          exactly 0.  One __ballot; the rows that pass -- a handful per chunk -- are queued in ascending row,
//                          lane p of the wave holding the p-th queued row (every lane finds its row in the ballot word by
//                          itself: no lane writes to another).
//                      (2) FLUSH, when 64 rows are queued and at the end: every queued row's iou3d::iou_bev(detection,
//                          candidate), is_member of box_fuse_core.h, one __ballot of the membership word.  The eight float64
//                          sums are then taken SERIALLY over the set bits, lowest first -- lane q < 8 owns sum q and receives
//                          the member's fields by shuffles.
//                      The queue keeps the rows ascending and the flushes follow one another, so the members are added in
//                      ascending candidate row whatever the chunking is: no tree, no atomics, no LDS, a pure function of the
//                      inputs.  Lanes 0..6 store the seven fields of the fused row.
//   scores_kernel      the score of a logit, one thread each: what the rule's numpy statement takes as its weights.
//
// Plain loads, shuffles and vector stores; no workspace, no memset, no workgroup waits for another.
#include "box_fuse_core.h"
#include "common.h"
#include "iou3d_device.h"
#include "sigmoid.h"

namespace {
using namespace sassd_fuse;

constexpr int kWaves = 4;

struct FuseArgs {
    const float *guided, *logits;
    const int32_t *labels, *counts;
    const float *det_boxes;
    const int32_t *det_labels, *det_counts;
    float *fused;
    int capK, capD;
    float score_thr, fuse_iou;
};

// (x - w/2, y - l/2, x + w/2, y + l/2, yaw): the BEV box rescore_prep_kernel builds
__device__ __forceinline__ iou3d::Box bev(const float *g)
{
    const float hx = g[3] / 2, hy = g[4] / 2;
    iou3d::Box b;
    b.x1 = g[0] - hx; b.y1 = g[1] - hy; b.x2 = g[0] + hx; b.y2 = g[1] + hy; b.r = g[6];
    return b;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// position of the r-th (0-based) set bit of w; r < popcount(w)
__device__ __forceinline__ int nth_set_bit(unsigned long long w, int r)
{
    int pos = 0;
#pragma unroll
    for (int width = 32; width >= 1; width >>= 1) {
        const int c = __popcll((w >> pos) & ((1ull << width) - 1ull));
        if (r >= c) { r -= c; pos += width; }
    }
    return pos;
}

__global__ void __launch_bounds__(kWaves * 64) box_fuse_kernel(FuseArgs a)
{
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int t = blockIdx.x * kWaves + (threadIdx.x >> 6);         // detection row: one per wave
    if (t >= clampi(a.det_counts[b], a.capD)) return;               // wave-uniform; rows at and past the count are not written
    const int K = clampi(a.counts[b], a.capK);
    const size_t row = (size_t)b * a.capD + t;
    float d[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) d[q] = a.det_boxes[row * 7 + q];
    const int label_d = a.det_labels[row];
    const iou3d::Box D = bev(d);
    const float dcx = (D.x1 + D.x2) * 0.5f, dcy = (D.y1 + D.y2) * 0.5f, wd = D.x2 - D.x1, ld = D.y2 - D.y1;
    const float rd = sqrtf(wd * wd + ld * ld);
    const float *guided = a.guided + (size_t)b * a.capK * 7;
    const float *logits = a.logits + (size_t)b * a.capK;
    const int32_t *labels = a.labels + (size_t)b * a.capK;

    double sum = 0.0;               // lane q < 8: sum q of box_fuse_core.h
    int members = 0;                // wave-uniform
    int queued = 0, qrow = 0;       // wave-uniform: rows in the queue; lane p < queued: its row, ascending in p

    // step (2): the rotated IoU of the queued rows, the membership word, the serial sums
    auto flush = [&]() {
        float s = 0.f, f[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        bool member = false;
        if (lane < queued) {                                        // qrow < K: it came out of a ballot of rows below K
            s = sigmoidf(logits[qrow]);
#pragma unroll
            for (int q = 0; q < 7; ++q) f[q] = guided[(size_t)qrow * 7 + q];
            member = is_member(s, a.score_thr, labels[qrow], label_d, iou3d::iou_bev(D, bev(f)), a.fuse_iou);
        }
        unsigned long long word = __ballot(member);
        while (word) {                                              // ascending lane = ascending candidate row
            const int i = __ffsll(word) - 1;
            word &= word - 1;
            const float sj = __shfl(s, i);
            float v = 0.f;
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                const float fq = __shfl(f[q], i);
                if (lane == q) v = fq;
            }
            if (lane < kSums) sum = add(sum, members == 0, term(lane, sj, v, d[6]));
            ++members;
        }
        queued = 0;
    };

    // step (1): the cheap two of is_member's three tests and the circle screen, 64 rows at a time
    for (int j0 = 0; j0 < K; j0 += 64) {
        const int j = j0 + lane;
        bool pass = false;
        if (j < K && labels[j] == label_d && sigmoidf(logits[j]) > a.score_thr) {
            const float *g = guided + (size_t)j * 7;
            const float f[7] = {g[0], g[1], 0.f, g[3], g[4], 0.f, 0.f};
            const iou3d::Box C = bev(f);
            // boxes whose circumscribed circles are disjoint (with slack) have overlap exactly 0 (nms_word of heads.hip):
            // IoU 0 >= fuse_iou is false for every fuse_iou > 0.  A NaN compares false and goes on to iou_bev
            const float dx = dcx - (C.x1 + C.x2) * 0.5f, dy = dcy - (C.y1 + C.y2) * 0.5f;
            const float wc = C.x2 - C.x1, lc = C.y2 - C.y1;
            const float rr = 0.5f * (rd + sqrtf(wc * wc + lc * lc)) + 1e-3f;
            pass = !(dx * dx + dy * dy > rr * rr);
        }
        const unsigned long long word = __ballot(pass);
        const int cnt = __popcll(word);
        for (int taken = 0; taken < cnt;) {                         // wave-uniform; twice only when the queue fills up
            const int take = min(64 - queued, cnt - taken);
            const int r = lane - queued;
            if (r >= 0 && r < take) qrow = j0 + nth_set_bit(word, taken + r);
            queued += take;
            taken += take;
            if (queued == 64) flush();
        }
    }
    if (queued) flush();
    const double W = __shfl(sum, kWeight);
    if (lane < 7) {
        uint32_t out = reinterpret_cast<const uint32_t *>(a.det_boxes)[row * 7 + lane];       // no fusable member: bit for bit
        if (fusable(members, W)) out = __float_as_uint(fused_field(lane, sum, W, d[6]));
        reinterpret_cast<uint32_t *>(a.fused)[row * 7 + lane] = out;
    }
}

__global__ void __launch_bounds__(256) scores_kernel(const float *__restrict__ logits, long long n, float *__restrict__ out)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = sigmoidf(logits[i]);
}
}  // namespace

extern "C" int sassd_box_fuse(const float *guided, const float *logits, const int32_t *labels, const int32_t *counts,
                              int batch, int capK, float score_thr, float fuse_iou, const float *det_boxes,
                              const int32_t *det_labels, const int32_t *det_counts, int capD, float *fused, void *stream_)
{
    if (!guided || !logits || !labels || !counts || !det_boxes || !det_labels || !det_counts || !fused) return SASSD_EINVAL;
    if (((uintptr_t)guided | (uintptr_t)logits | (uintptr_t)labels | (uintptr_t)counts | (uintptr_t)det_boxes |
         (uintptr_t)det_labels | (uintptr_t)det_counts | (uintptr_t)fused) & 3)
        return SASSD_EINVAL;
    if (batch < 1 || batch > 65535 || capK < 1 || capK > 4096 || capD < 1) return SASSD_EINVAL;
    if (!(fuse_iou > 0.f && fuse_iou < 1.f)) return SASSD_EINVAL;               // NaN and the infinities included
    if ((long long)batch * capD > 0x7fffffff / 7) return SASSD_EINVAL;
    const size_t n = (size_t)batch * capD * 7;
    if (fused < det_boxes + n && det_boxes < fused + n) return SASSD_EINVAL;    // not in place: the detections stay readable
    FuseArgs a;
    a.guided = guided; a.logits = logits; a.labels = labels; a.counts = counts;
    a.det_boxes = det_boxes; a.det_labels = det_labels; a.det_counts = det_counts; a.fused = fused;
    a.capK = capK; a.capD = capD; a.score_thr = score_thr; a.fuse_iou = fuse_iou;
    hipLaunchKernelGGL(box_fuse_kernel, dim3(cdiv(capD, kWaves), batch), dim3(kWaves * 64), 0, (hipStream_t)stream_, a);
    return sassd_launch_status();
}

extern "C" int sassd_candidate_scores(const float *logits, long long n, float *scores, void *stream_)
{
    if (!logits || !scores || (((uintptr_t)logits | (uintptr_t)scores) & 3)) return SASSD_EINVAL;
    if (n < 0 || n > (long long)0x7fffffff * 256) return SASSD_EINVAL;
    if (n == 0) return SASSD_OK;
    hipLaunchKernelGGL(scores_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream_, logits, n, scores);
    return sassd_launch_status();
}
