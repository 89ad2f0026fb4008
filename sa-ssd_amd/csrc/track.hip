// track.hip -- identity across frames (include/sassd.h "Tracking"): a greedy centre-distance tracker behind a frame's
// detections.  The rule is track_core.h; this file is its schedule.
//
//   track_kernel   ONE WORKGROUP of 256 threads per sample, one launch per frame.  The sample's slot table (<= 1024 slots of 56
//                  bytes) is loaded into LDS word-major -- word w of slot i at tab[w][i], so that the threads of a wave touch
//                  consecutive banks -- and thread t owns the slots i = t, t + 256, ... from then on:
//                  (1) reset / predict: every thread on its own slots.
//                  (2) associate: the detections one after the other, in the detector's order, staged in LDS 64 at a time so
//                      that the serial loop makes one trip to memory per 64 detections.  Per detection every thread scans
//                      its own slots for the eligible one of least cost (ascending slot, strict <, so the lowest slot wins a tie),
//                      the 64 lanes of a wave reduce the (cost, slot) pairs by xor shuffles under the same order, lane 0 of each
//                      of the four waves leaves its pair in LDS, and behind ONE barrier every thread reads the four pairs and
//                      knows the winner.  The owner of the winning slot updates it; no other thread reads that slot before
//                      the loop ends, so the update needs no barrier of its own.  The four pairs are double-buffered by the
//                      parity of the detection: a thread that writes buffer p for detection d + 2 has passed the barrier of
//                      d + 1, behind which nobody reads the pairs of d any more.  Thread d % 256 keeps "detection d found a
//                      track" as bit d / 256 of a register.
//                  (3) age: every thread on its own slots.  Then the free slots are listed in ascending order (a block scan over
//                      each pass of 256 slots), the detections that give birth are ranked in ascending order (a block scan
//                      over each chunk of 256 detections), and the r-th birth takes the r-th free slot and the id next_id + r:
//                      the order of the rule, without a serial loop.  Births past the free list are counted as dropped.
//                  (4) write back: the table to the state and to the record, the rows of the detections from their slots.  A
//                      detection row is written by exactly one thread: the owner of its slot, or -- when it has none -- the
//                      thread that ranked it.
//
// Plain loads, shuffles, LDS and vector stores: no atomics, no memset, no workspace, no workgroup waits for another.
#include "common.h"
#include "track_core.h"

namespace {
using namespace sassd_track;

constexpr int kThreads = 256, kWaves = kThreads / 64, kStage = 64;

struct TrackArgs {
    const int32_t *boxes, *scores;              // the detections, as 32-bit words: they are copied bit for bit
    const int32_t *labels, *counts, *seq, *status;
    const Desc *desc;
    int32_t *slots, *next_id;
    int32_t *record;
    int B, capD, cap, n_labels, max_age;
    float birth_score;
    double alpha;
    double gate[kMaxLabels];
};

struct LdsTab {
    int32_t (*p)[kMaxCap];
    __device__ __forceinline__ int32_t &w(int word, int slot) { return p[word][slot]; }
};

__global__ void __launch_bounds__(kThreads) track_kernel(TrackArgs a)
{
    __shared__ int32_t tab_[kSlotWords][kMaxCap];       // 56 KB
    __shared__ int16_t s_det[kMaxCap];                  // the detection slot i took in this frame (matched or born), or -1
    __shared__ int16_t s_free[kMaxCap];                 // the free slots behind step 5, ascending
    __shared__ double red_c[2][kWaves];
    __shared__ int red_i[2][kWaves];
    __shared__ int wsum[17];
    __shared__ int32_t s_box[kStage][7], s_score[kStage], s_label[kStage];      // the staged detections

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int cap = a.cap, capD = a.capD;
    LdsTab tab{tab_};
    const Desc desc = a.desc[b];
    const int st = a.status[0];
    const int32_t id0 = a.next_id[b];
    int32_t *gslots = a.slots + (size_t)b * cap * kSlotWords;
    const size_t drow = (size_t)b * capD;

    for (int j = tid; j < cap * kSlotWords; j += kThreads) tab_[j % kSlotWords][j / kSlotWords] = gslots[j];
    __syncthreads();
    // steps 1 and 2, every thread on the slots it owns
    for (int i = tid; i < cap; i += kThreads) {
        s_det[i] = -1;
        if (desc.flags & 1) tab.w(kId, i) = -1;
        else if (tab.w(kId, i) >= 0) predict(tab, i, desc);
    }
    const bool flagged = st != 0;                       // the tracks are carried along, nothing else happens
    int D = flagged ? 0 : a.counts[b];
    D = D < 0 ? 0 : (D > capD ? capD : D);

    // step 3 with step 4
    unsigned long long found = 0;                       // bit c: detection c * 256 + tid found a track
    for (int d0 = 0; d0 < D; d0 += kStage) {            // the detections are staged kStage at a time: one trip to memory each
        const int nd = D - d0 < kStage ? D - d0 : kStage;
        __syncthreads();                                // the last update of the chunk before has read its detection
        for (int j = tid; j < nd * 7; j += kThreads) (&s_box[0][0])[j] = a.boxes[(drow + d0) * 7 + j];
        if (tid < nd) { s_score[tid] = a.scores[drow + d0 + tid]; s_label[tid] = a.labels[drow + d0 + tid]; }
        __syncthreads();
        for (int k = 0; k < nd; ++k) {
            const int d = d0 + k;
            const float x = f_of(s_box[k][0]), y = f_of(s_box[k][1]);
            const int label = s_label[k];
            double bc = 0.0;
            int bi = kNone;
            if (label >= 0 && label < a.n_labels) {
                const double gate = a.gate[label];
                for (int i = tid; i < cap; i += kThreads) {
                    if (tab.w(kId, i) < 0 || s_det[i] >= 0 || tab.w(kLabel, i) != label) continue;
                    const double c = cost(x, y, f_of(tab.w(kBox + 0, i)), f_of(tab.w(kBox + 1, i)));
                    if (eligible(c, gate) && (bi == kNone || better(c, i, bc, bi))) { bc = c; bi = i; }
                }
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const double oc = __shfl_xor(bc, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (oi != kNone && (bi == kNone || better(oc, oi, bc, bi))) { bc = oc; bi = oi; }
            }
            const int p = d & 1;
            if (lane == 0) { red_c[p][wid] = bc; red_i[p][wid] = bi; }
            __syncthreads();
            bc = red_c[p][0]; bi = red_i[p][0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) {
                const double oc = red_c[p][w];
                const int oi = red_i[p][w];
                if (oi != kNone && (bi == kNone || better(oc, oi, bc, bi))) { bc = oc; bi = oi; }
            }
            if (bi != kNone) {
                if ((d & (kThreads - 1)) == tid) found |= 1ull << (d / kThreads);
                if ((bi & (kThreads - 1)) == tid) {     // the owner of the winning slot
                    update(tab, bi, s_box[k], s_score[k], desc, a.alpha);
                    s_det[bi] = (int16_t)d;
                }
            }
        }
    }

    // steps 5 and 6
    int nfree = 0;
    if (!flagged) {
        for (int i0 = 0; i0 < cap; i0 += kThreads) {    // block-uniform trip count
            const int i = i0 + tid;
            int free_ = 0;
            if (i < cap) {
                if (tab.w(kId, i) >= 0 && s_det[i] < 0) age(tab, i, a.max_age);
                free_ = tab.w(kId, i) < 0;
            }
            int total;
            const int r = nfree + block_exclusive_scan(free_, wsum, &total);
            if (free_) s_free[r] = (int16_t)i;
            nfree += total;
        }
        __syncthreads();                                // the free list is complete
    }
    const RecordLayout L = record_layout(a.B, capD, cap);
    int32_t *rec = a.record;
    int births = 0;                                     // detections that give birth, those past the free list included
    for (int d0 = 0; d0 < capD; d0 += kThreads) {       // block-uniform trip count; rows at and past D only get their -1 / 0 / 0
        const int d = d0 + tid;
        const bool has = (found >> (d0 / kThreads)) & 1ull;
        int cand = 0;
        if (d < D && !has) cand = gives_birth(f_of(a.scores[drow + d]), a.birth_score);
        int total;
        const int r = births + block_exclusive_scan(cand, wsum, &total);
        births += total;
        bool born = false;
        if (cand && r < nfree) {
            const int i = s_free[r];
            birth(tab, i, (int32_t)((uint32_t)id0 + (uint32_t)r), a.labels[drow + d], a.boxes + (drow + d) * 7, a.scores[drow + d]);
            s_det[i] = (int16_t)d;
            born = true;
        }
        if (d < capD && !has && !born) {                // no slot will write this row
            rec[L.det_id + drow + d] = -1;
            rec[L.det_hits + drow + d] = 0;
            rec[L.det_vel + 2 * (drow + d)] = 0;
            rec[L.det_vel + 2 * (drow + d) + 1] = 0;
        }
    }
    __syncthreads();                                    // the newborn slots are in the table
    const int born_n = births < nfree ? births : nfree;

    // write back
    for (int i = tid; i < cap; i += kThreads) {
        const int d = s_det[i];
        if (d < 0) continue;
        rec[L.det_id + drow + d] = tab.w(kId, i);
        rec[L.det_hits + drow + d] = tab.w(kHits, i);
        rec[L.det_vel + 2 * (drow + d)] = tab.w(kVel + 0, i);
        rec[L.det_vel + 2 * (drow + d) + 1] = tab.w(kVel + 1, i);
    }
    int32_t *rslots = rec + L.slots + (size_t)b * cap * kSlotWords;
    for (int j = tid; j < cap * kSlotWords; j += kThreads) {
        const int32_t v = tab_[j % kSlotWords][j / kSlotWords];
        gslots[j] = v;
        rslots[j] = v;
    }
    if (tid == 0) {
        const int32_t next = (int32_t)((uint32_t)id0 + (uint32_t)born_n);
        a.next_id[b] = next;
        rec[L.count + b] = D;
        rec[L.dropped + b] = births - born_n;
        rec[L.next_id + b] = next;
    }
    if (b == 0 && tid == 0) {
        rec[0] = (int32_t)kMagic; rec[1] = a.seq[0]; rec[2] = st; rec[3] = a.B; rec[4] = capD; rec[5] = cap;
        rec[6] = 0; rec[7] = 0;
    }
}
}  // namespace

extern "C" size_t sassd_track_record_bytes(int batch, int capD, int cap)
{
    if (batch < 1 || batch > 65535 || capD < 1 || capD > sassd_track::kMaxCapD || cap < 1 || cap > sassd_track::kMaxCap) return 0;
    return 4 * sassd_track::record_layout(batch, capD, cap).total;
}

extern "C" int sassd_track_step(const float *det_boxes, const float *det_scores, const int32_t *det_labels,
                                const int32_t *det_counts, int batch, int capD, const int32_t *seq, const int32_t *status,
                                const void *desc, int32_t *slots, int32_t *next_id, int cap, const float *max_dist, int n_labels,
                                int max_age, double alpha, float birth_score, void *record, size_t record_bytes, void *stream_)
{
    if (!det_boxes || !det_scores || !det_labels || !det_counts || !seq || !status || !desc || !slots || !next_id || !max_dist ||
        !record)
        return SASSD_EINVAL;
    if (((uintptr_t)det_boxes | (uintptr_t)det_scores | (uintptr_t)det_labels | (uintptr_t)det_counts | (uintptr_t)seq |
         (uintptr_t)status | (uintptr_t)slots | (uintptr_t)next_id | (uintptr_t)record) & 3)
        return SASSD_EINVAL;
    if ((uintptr_t)desc & 7) return SASSD_EINVAL;
    if (batch < 1 || batch > 65535 || capD < 1 || capD > kMaxCapD || cap < 1 || cap > kMaxCap) return SASSD_EINVAL;
    if (n_labels < 1 || n_labels > kMaxLabels || max_age < 0) return SASSD_EINVAL;
    if (!(alpha > 0.0 && alpha <= 1.0)) return SASSD_EINVAL;                    // NaN included
    if (birth_score != birth_score) return SASSD_EINVAL;
    TrackArgs a;
    for (int l = 0; l < kMaxLabels; ++l) {
        const float m = max_dist[l < n_labels ? l : n_labels - 1];
        if (!(m >= 0.f && m <= 3.4028234663852886e38f)) return SASSD_EINVAL;   // negative, NaN, infinite
        a.gate[l] = gate2(m);
    }
    if (record_bytes < sassd_track_record_bytes(batch, capD, cap)) return SASSD_ENOSPC;
    a.boxes = reinterpret_cast<const int32_t *>(det_boxes); a.scores = reinterpret_cast<const int32_t *>(det_scores);
    a.labels = det_labels; a.counts = det_counts; a.seq = seq; a.status = status;
    a.desc = static_cast<const Desc *>(desc); a.slots = slots; a.next_id = next_id; a.record = static_cast<int32_t *>(record);
    a.B = batch; a.capD = capD; a.cap = cap; a.n_labels = n_labels; a.max_age = max_age;
    a.birth_score = birth_score; a.alpha = alpha;
    hipLaunchKernelGGL(track_kernel, dim3(batch), dim3(kThreads), 0, (hipStream_t)stream_, a);
    return sassd_launch_status();
}
