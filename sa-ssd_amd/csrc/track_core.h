// track_core.h -- the rule of the greedy centre-distance tracker (include/sassd.h "Tracking"), stated once: how a track is
// carried into the current sensor frame, what a detection may be matched with and which slot wins, how a matched slot is
// updated, how an unmatched one ages, and what a newborn track holds.  Written as __host__ __device__ functions so that the very
// same text is (a) called by the threads of track.hip and (b) looped over on the CPU by tests/track_harness.hip, which checks it
// against the numpy statement sassd.track.track_host without a GPU.
//
// A slot is kSlotWords 32-bit words; the functions reach it through a table `Tab` with `int32_t &w(int word, int slot)`, so the
// kernel's LDS table (word-major) and the harness's memory image (slot-major) run the same lines.  All arithmetic is float64 on
// the float32 fields, every product, quotient and sum is rounded on its own (no fused multiply-add), results are stored as
// float32: the state after a step is a pure function of the state before it, the detections and the descriptor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sassd_track {

constexpr int kSlotWords = 14;                  // id | label | box[7] | vel[2] | hits | misses | score
constexpr int kId = 0, kLabel = 1, kBox = 2, kVel = 9, kHits = 11, kMisses = 12, kScore = 13;
constexpr int kMaxCap = 1024, kMaxLabels = 8, kMaxCapD = 16384, kMaxHits = 1 << 30;
constexpr int kNone = 0x7fffffff;               // "no slot": loses against every slot in better()

// the per-frame descriptor of one sample, made on the host (sassd.track.pack_desc): no trigonometry is left for the device
struct Desc {
    double T[12];                               // sweep_transform(pose_now, pose_prev), [3,4] row-major
    double dyaw, dt;                            // atan2(T[1,0], T[0,0]);  time_now - time_prev
    int32_t flags, pad;                         // bit 0: reset (the first frame of a sequence)
};
static_assert(sizeof(Desc) == 120, "the descriptor is 120 bytes");

__host__ __device__ inline float f_of(int32_t w) { float f; __builtin_memcpy(&f, &w, 4); return f; }
__host__ __device__ inline int32_t w_of(float f) { int32_t w; __builtin_memcpy(&w, &f, 4); return w; }

// one row of T applied to (px, py, pz), rounded to float32 at the end
__host__ __device__ inline float row_apply(const double *r, double px, double py, double pz)
{
#pragma clang fp contract(off)
    return (float)(((r[0] * px + r[1] * py) + r[2] * pz) + r[3]);
}

// step 2: a live slot moved by its velocity over dt, then into the current sensor frame; the sizes stay
template <class Tab> __host__ __device__ inline void predict(Tab &t, int i, const Desc &d)
{
#pragma clang fp contract(off)
    const double x = f_of(t.w(kBox + 0, i)), y = f_of(t.w(kBox + 1, i)), z = f_of(t.w(kBox + 2, i));
    const double yaw = f_of(t.w(kBox + 6, i)), vx = f_of(t.w(kVel + 0, i)), vy = f_of(t.w(kVel + 1, i));
    const double px = x + vx * d.dt, py = y + vy * d.dt, pz = z;
    t.w(kBox + 0, i) = w_of(row_apply(d.T + 0, px, py, pz));
    t.w(kBox + 1, i) = w_of(row_apply(d.T + 4, px, py, pz));
    t.w(kBox + 2, i) = w_of(row_apply(d.T + 8, px, py, pz));
    t.w(kBox + 6, i) = w_of((float)(yaw + d.dyaw));
    t.w(kVel + 0, i) = w_of((float)(d.T[0] * vx + d.T[1] * vy));
    t.w(kVel + 1, i) = w_of((float)(d.T[4] * vx + d.T[5] * vy));
}

// step 3: the squared gate of a label, the cost of (detection, slot), and the order of two (cost, slot) pairs
__host__ __device__ inline double gate2(float max_dist)
{
#pragma clang fp contract(off)
    const double m = (double)max_dist;
    return m * m;
}

__host__ __device__ inline double cost(float det_x, float det_y, float x, float y)
{
#pragma clang fp contract(off)
    const double dx = (double)det_x - (double)x, dy = (double)det_y - (double)y;
    return dx * dx + dy * dy;
}

// a NaN cost is not eligible (the comparison is false)
__host__ __device__ inline bool eligible(double c, double gate) { return c <= gate; }

// (c, i) beats (cb, ib): the least cost, on equal cost the lowest slot.  Costs here are eligible, so never NaN
__host__ __device__ inline bool better(double c, int i, double cb, int ib) { return c < cb || (c == cb && i < ib); }

// step 4: the velocity moves only over a finite, positive dt
__host__ __device__ inline bool dt_usable(double dt) { return dt > 0.0 && dt <= 1.7976931348623157e308; }

__host__ __device__ inline float vel_update(float v_pred, float det, float pred, double dt, double g)
{
#pragma clang fp contract(off)
    const double r = ((double)det - (double)pred) / dt;
    return (float)((double)v_pred + g * r);
}

// step 4: slot i takes detection (box words, score word); the box and the score bit for bit
template <class Tab>
__host__ __device__ inline void update(Tab &t, int i, const int32_t *det_box, int32_t det_score, const Desc &d, double alpha)
{
    const int hits = t.w(kHits, i);
    const double g = hits == 1 ? 1.0 : alpha;
    if (dt_usable(d.dt)) {
        const float vx = vel_update(f_of(t.w(kVel + 0, i)), f_of(det_box[0]), f_of(t.w(kBox + 0, i)), d.dt, g);
        const float vy = vel_update(f_of(t.w(kVel + 1, i)), f_of(det_box[1]), f_of(t.w(kBox + 1, i)), d.dt, g);
        t.w(kVel + 0, i) = w_of(vx);
        t.w(kVel + 1, i) = w_of(vy);
    }
    for (int q = 0; q < 7; ++q) t.w(kBox + q, i) = det_box[q];
    t.w(kScore, i) = det_score;
    t.w(kHits, i) = hits + 1 < kMaxHits ? hits + 1 : kMaxHits;
    t.w(kMisses, i) = 0;
}

// step 5: a live slot that no detection took
template <class Tab> __host__ __device__ inline void age(Tab &t, int i, int max_age)
{
    const int m = t.w(kMisses, i) + 1;
    t.w(kMisses, i) = m;
    if (m > max_age) t.w(kId, i) = -1;
}

// step 6: which detections found a track, and what the newborn holds.  A NaN score gives no birth
__host__ __device__ inline bool gives_birth(float score, float birth_score) { return score >= birth_score; }

template <class Tab>
__host__ __device__ inline void birth(Tab &t, int i, int32_t id, int32_t label, const int32_t *det_box, int32_t det_score)
{
    t.w(kId, i) = id;
    t.w(kLabel, i) = label;
    for (int q = 0; q < 7; ++q) t.w(kBox + q, i) = det_box[q];
    t.w(kVel + 0, i) = 0;
    t.w(kVel + 1, i) = 0;
    t.w(kHits, i) = 1;
    t.w(kMisses, i) = 0;
    t.w(kScore, i) = det_score;
}

// ---- the device record (include/sassd.h "Tracking"; sassd.track.track_record_layout is its Python statement) -----------
constexpr uint32_t kMagic = 0x53540001u;        // SASSD_TRACK_MAGIC: 'S' 'T', layout version 1
constexpr int kHeaderWords = 8;                 // magic, seq, status, B, capD, cap, 0, 0

struct RecordLayout { size_t count, dropped, next_id, det_id, det_hits, det_vel, slots, total; };     // in 32-bit words

__host__ __device__ inline RecordLayout record_layout(int B, int capD, int cap)
{
    RecordLayout L;
    const size_t b = (size_t)B, n = b * (size_t)capD;
    L.count = kHeaderWords;
    L.dropped = L.count + b;
    L.next_id = L.dropped + b;
    L.det_id = L.next_id + b;
    L.det_hits = L.det_id + n;
    L.det_vel = L.det_hits + n;
    L.slots = L.det_vel + 2 * n;
    L.total = L.slots + b * (size_t)cap * kSlotWords;
    return L;
}

}  // namespace sassd_track
