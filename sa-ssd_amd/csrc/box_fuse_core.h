// box_fuse_core.h -- the rule of box fusion (include/sassd.h "Box fusion"), stated once: which candidates are members of a
// detection, what a member adds to each of the eight float64 sums, and how the sums become the fused box.  Written as
// __host__ __device__ functions so that the very same text is (a) called by the lanes of box_fuse.hip and (b) looped over on
// the CPU by tests/box_fuse_harness.hip, which checks it against the numpy statement sassd.fuse.fuse_host without a GPU.
//
// The score s of a candidate (sigmoidf of sigmoid.h on its logit) and its rotated BEV IoU with the detection
// (iou3d::iou_bev(bev(detection), bev(candidate))) are inputs here: both are device functions.  Everything below is
// float64, every product, quotient and sum is rounded on its own (no fused multiply-add), and the members are taken in
// ascending candidate row, so the result is a pure function of the inputs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sassd_fuse {

constexpr int kSums = 8;            // sum q: 0..5 the score-weighted x, y, z, w, l, h; 6 the weighted heading offset; 7 W
constexpr int kYaw = 6, kWeight = 7;

// candidate (score s, label, IoU with the detection) is a member of a detection of label `label_d`.  A NaN score or a NaN
// IoU is not a member (both comparisons are false).
__host__ __device__ inline bool is_member(float s, float score_thr, int label, int label_d, float iou, float fuse_iou)
{
    return s > score_thr && label == label_d && iou >= fuse_iou;
}

// the heading of a member relative to the detection's, folded into [-pi/2, pi/2): a rectangle pointing the opposite way is
// the same rectangle and must not drag the heading round
__host__ __device__ inline double yaw_delta(float yaw, float yaw_d)
{
#pragma clang fp contract(off)
    const double pi = 3.14159265358979323846;
    const double d = (double)yaw - (double)yaw_d;
    const double k = floor(d / pi + 0.5);
    return d - pi * k;
}

// what a member adds to sum q; v is its field q (its yaw for q = 6, unused for q = 7).  s * v is exact for q < 6
__host__ __device__ inline double term(int q, float s, float v, float yaw_d)
{
#pragma clang fp contract(off)
    if (q == kWeight) return (double)s;
    if (q == kYaw) return (double)s * yaw_delta(v, yaw_d);
    return (double)s * (double)v;
}

// the sum after one more member: the sum of one term is the term (so that a field of -0.0 stays -0.0)
__host__ __device__ inline double add(double sum, bool first, double t)
{
#pragma clang fp contract(off)
    return first ? t : sum + t;
}

// the fused box exists: at least one member and a positive finite W; otherwise the detection is returned as it is
__host__ __device__ inline bool fusable(int members, double W) { return members > 0 && W > 0.0 && W <= 1.7976931348623157e308; }

// field q (0..6) of the fused box from sum q and W
__host__ __device__ inline float fused_field(int q, double sum, double W, float yaw_d)
{
#pragma clang fp contract(off)
    const double m = sum / W;
    return q == kYaw ? (float)((double)yaw_d + m) : (float)m;
}

}  // namespace sassd_fuse
