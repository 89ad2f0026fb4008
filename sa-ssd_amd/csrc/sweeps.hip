// sweeps.hip -- merge of the current LiDAR sweep with up to 15 earlier ones, each moved into the current sensor frame by
// its ego-pose transform, the time lag as an optional last feature: the FIRST node of a captured frame whose stream keeps
// its sweeps in a device ring (include/sassd.h "Multi-sweep merge").  The merged cloud is what the voxelizer reads next.
//
// One launch, grid (ceil(sweep_cap / 256), S): workgroup (x, s) owns rows x * 256 .. x * 256 + 255 of entry s.  Every
// thread reads the S <= 16 descriptor words of the frame (wave-uniform: scalar loads), sums the clamped counts of the
// entries before its own -- its entry's first output row -- and moves its one row.  No workgroup waits for another and
// nothing is counted across workgroups: the output order (entry 0 first, ascending rows within an entry) follows from
// the counts alone.  Traffic per merged row: ndim_in floats read, ndim_out floats written.
#include "common.h"

namespace {

constexpr int kThreads = 256, kMaxSweeps = 16;

struct SweepArgs {
    const float *ring;
    const int32_t *slot, *count, *xform;
    const double *T;
    const float *dt;
    float *out;
    int32_t *n_out, *status;
    int R, sweep_cap, ndim_in, S, time_feature, cap_out;
};

// rows entry j contributes: its count clamped to [0, sweep_cap], 0 for a slot outside the ring
__device__ __forceinline__ int entry_rows(const SweepArgs &a, int j)
{
    const int sl = a.slot[j], c = a.count[j];
    if (sl < 0 || sl >= a.R || c <= 0) return 0;
    return c > a.sweep_cap ? a.sweep_cap : c;
}

// xyz of a row in the current sensor frame: float64, every product and sum rounded separately, in this order
__device__ __forceinline__ void move_xyz(const double *T, float &x, float &y, float &z)
{
#pragma clang fp contract(off)
    const double dx = (double)x, dy = (double)y, dz = (double)z;
    const double ox = T[0] * dx + T[1] * dy + T[2] * dz + T[3];
    const double oy = T[4] * dx + T[5] * dy + T[6] * dz + T[7];
    const double oz = T[8] * dx + T[9] * dy + T[10] * dz + T[11];
    x = (float)ox;
    y = (float)oy;
    z = (float)oz;
}

template <bool VEC4>
__global__ void __launch_bounds__(kThreads) merge_sweeps_kernel(SweepArgs a)
{
    const int s = blockIdx.y;                                   // < S by the grid
    long long base = 0, total = 0;
    int mine = 0;
    bool over = false;
    for (int j = 0; j < a.S; ++j) {
        const int c = entry_rows(a, j);
        if (j < s) base += c;
        if (j == s) mine = c;
        total += c;
        over |= a.count[j] > a.sweep_cap;
    }
    if (blockIdx.x == 0 && s == 0 && threadIdx.x == 0) {
        *a.n_out = total < (long long)a.cap_out ? (int32_t)total : a.cap_out;
        if (over || total > (long long)a.cap_out) atomicOr(a.status, SASSD_ST_POINT_OVERFLOW);
    }
    const long long r = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= mine) return;                                      // mine > 0: slot[s] is inside the ring
    const long long o = base + r;
    if (o >= (long long)a.cap_out) return;
    const size_t src_row = ((size_t)a.slot[s] * (size_t)a.sweep_cap + (size_t)r);
    const bool moved = a.xform[s] != 0;
    const double *T = a.T + 12 * s;
    if (VEC4) {
        float4 v = reinterpret_cast<const float4 *>(a.ring)[src_row];
        if (moved) move_xyz(T, v.x, v.y, v.z);
        reinterpret_cast<float4 *>(a.out)[o] = v;
        return;
    }
    const int nd_out = a.ndim_in + (a.time_feature ? 1 : 0);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(a.ring) + src_row * (size_t)a.ndim_in;
    uint32_t *dst = reinterpret_cast<uint32_t *>(a.out) + (size_t)o * (size_t)nd_out;
    if (moved) {
        float x = __uint_as_float(src[0]), y = __uint_as_float(src[1]), z = __uint_as_float(src[2]);
        move_xyz(T, x, y, z);
        dst[0] = __float_as_uint(x);
        dst[1] = __float_as_uint(y);
        dst[2] = __float_as_uint(z);
    } else {
        dst[0] = src[0];
        dst[1] = src[1];
        dst[2] = src[2];
    }
    for (int c = 3; c < a.ndim_in; ++c) dst[c] = src[c];
    if (a.time_feature) dst[a.ndim_in] = __float_as_uint(a.dt[s]);
}
}  // namespace

extern "C" int sassd_merge_sweeps_dev(const float *ring, int R, int sweep_cap, int ndim_in, const int32_t *slot,
                                      const int32_t *count, const int32_t *xform, const double *T, const float *dt, int S,
                                      int time_feature, float *out, int cap_out, int32_t *n_out_dev, int32_t *status,
                                      void *stream_)
{
    if (!ring || !slot || !count || !xform || !T || !dt || !out || !n_out_dev || !status) return SASSD_EINVAL;
    if (S < 1 || S > kMaxSweeps || R < 1 || sweep_cap < 1 || cap_out < 1 || ndim_in < 3) return SASSD_EINVAL;
    if ((uintptr_t)T & 7) return SASSD_EINVAL;
    if (((uintptr_t)ring | (uintptr_t)slot | (uintptr_t)count | (uintptr_t)xform | (uintptr_t)dt | (uintptr_t)out |
         (uintptr_t)n_out_dev | (uintptr_t)status) & 3)
        return SASSD_EINVAL;
    SweepArgs a;
    a.ring = ring; a.slot = slot; a.count = count; a.xform = xform; a.T = T; a.dt = dt;
    a.out = out; a.n_out = n_out_dev; a.status = status;
    a.R = R; a.sweep_cap = sweep_cap; a.ndim_in = ndim_in; a.S = S; a.time_feature = time_feature ? 1 : 0; a.cap_out = cap_out;
    const dim3 grid((sweep_cap - 1) / kThreads + 1, S), block(kThreads);      // a function of (S, sweep_cap) alone
    hipStream_t s = (hipStream_t)stream_;
    if (ndim_in == 4 && !time_feature && ((((uintptr_t)ring | (uintptr_t)out) & 15) == 0))       // 16-byte row loads and stores
        hipLaunchKernelGGL(merge_sweeps_kernel<true>, grid, block, 0, s, a);
    else
        hipLaunchKernelGGL(merge_sweeps_kernel<false>, grid, block, 0, s, a);
    return sassd_launch_status();
}
