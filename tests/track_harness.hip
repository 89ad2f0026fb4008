// TEST INFRASTRUCTURE (never linked into libsassd.so, never imported by the product path).
// Loops the product's __host__ __device__ tracking rule on the CPU -- predict, gate2, cost, eligible, better, update, age,
// gives_birth and birth of sa-ssd_amd/csrc/track_core.h, serially, in the order the rule states (include/sassd.h "Tracking") --
// on a slot-major memory image of one sample's table, so that the arithmetic of the device path can be checked against
// sassd.track.track_host in the GPU-less test suite.
// Built host-only (hipcc -x hip --cuda-host-only) by tests/track_cases.py into a temporary directory.
#include "../sa-ssd_amd/csrc/track_core.h"

#include <vector>

namespace {
struct MemTab {
    int32_t *p;
    int32_t &w(int word, int slot) { return p[(size_t)slot * sassd_track::kSlotWords + word]; }
};
}  // namespace

// one sample, one step.  det_id / det_hits [capD] and det_vel [capD, 2] are written in full; out2 = {count, dropped}
extern "C" void hst_track_step(const int32_t *boxes, const int32_t *scores, const int32_t *labels, int count, int capD,
                               int status, const void *desc_, int32_t *slots, int32_t *next_id, int cap, const float *max_dist,
                               int n_labels, int max_age, double alpha, float birth_score, int32_t *det_id, int32_t *det_hits,
                               int32_t *det_vel, int32_t *out2)
{
    using namespace sassd_track;
    const Desc &desc = *static_cast<const Desc *>(desc_);
    MemTab t{slots};
    for (int d = 0; d < capD; ++d) { det_id[d] = -1; det_hits[d] = 0; det_vel[2 * d] = det_vel[2 * d + 1] = 0; }
    out2[0] = out2[1] = 0;
    for (int i = 0; i < cap; ++i) {
        if (desc.flags & 1) t.w(kId, i) = -1;
        else if (t.w(kId, i) >= 0) predict(t, i, desc);
    }
    if (status != 0) return;
    const int D = count < 0 ? 0 : (count > capD ? capD : count);
    out2[0] = D;
    std::vector<int> det_of(cap, -1), slot_of(D, -1);
    for (int d = 0; d < D; ++d) {
        const int label = labels[d];
        if (label < 0 || label >= n_labels) continue;
        const double gate = gate2(max_dist[label]);
        double bc = 0.0;
        int bi = kNone;
        for (int i = 0; i < cap; ++i) {
            if (t.w(kId, i) < 0 || det_of[i] >= 0 || t.w(kLabel, i) != label) continue;
            const double c = cost(f_of(boxes[d * 7]), f_of(boxes[d * 7 + 1]), f_of(t.w(kBox, i)), f_of(t.w(kBox + 1, i)));
            if (eligible(c, gate) && (bi == kNone || better(c, i, bc, bi))) { bc = c; bi = i; }
        }
        if (bi == kNone) continue;
        update(t, bi, boxes + d * 7, scores[d], desc, alpha);
        det_of[bi] = d;
        slot_of[d] = bi;
    }
    for (int i = 0; i < cap; ++i)
        if (t.w(kId, i) >= 0 && det_of[i] < 0) age(t, i, max_age);
    for (int d = 0; d < D; ++d) {
        if (slot_of[d] >= 0 || !gives_birth(f_of(scores[d]), birth_score)) continue;
        int i = 0;
        while (i < cap && t.w(kId, i) >= 0) ++i;
        if (i == cap) { ++out2[1]; continue; }
        birth(t, i, *next_id, labels[d], boxes + d * 7, scores[d]);
        *next_id = (int32_t)((uint32_t)*next_id + 1u);
        slot_of[d] = i;
    }
    for (int d = 0; d < D; ++d) {
        const int i = slot_of[d];
        if (i < 0) continue;
        det_id[d] = t.w(kId, i);
        det_hits[d] = t.w(kHits, i);
        det_vel[2 * d] = t.w(kVel, i);
        det_vel[2 * d + 1] = t.w(kVel + 1, i);
    }
}
