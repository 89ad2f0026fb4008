// crop.hip -- stable compaction of a raw LiDAR sweep to one convex polytope (the camera-2 viewing frustum), the first
// two nodes of a captured frame that starts at the raw sweep (include/sassd.h "Frustum crop").  The per-point test is
// inside_polytope of augment_core.h, the function the offline reduction (sassd_points_in_polytopes) evaluates, so the
// rows that survive are the rows of velodyne_reduced/, in the same order.
//
// Two launches, no waiting between workgroups.  A workgroup owns a fixed block of kBlock = 1024 rows: 4 passes of 256
// threads, thread t taking row block * 1024 + pass * 256 + t, so that a wave reads 64 consecutive rows.
//   count   every wave tests its 4 x 64 rows and writes how many it keeps to ws[block * 4 + wave] (waves past n write 0)
//   scatter every workgroup sums the counts of the blocks before it, tests its rows again, ranks the kept rows by
//           (pass, wave, lane) -- which is ascending row order -- and copies them to out[base + rank] while that is
//           below cap_out; the last workgroup writes *n_out and the overflow flag.
// Traffic for a 120 k-point sweep of 16-byte rows: 2 x 1.9 MB read (the second read hits L2), 16 B written per kept row,
// 1.9 KB of counts.  The time is the two launches.
#include "augment_core.h"
#include "common.h"

namespace {
using namespace sassd_aug;

constexpr int kThreads = 256, kPasses = 4, kBlock = kThreads * kPasses, kWaves = kThreads / SASSD_WAVE;

struct CropArgs {
    const float *pts;
    const int32_t *n_in;
    const double *planes;
    float *out;
    int32_t *n_out, *status, *counts;
    int cap_in, cap_out, ndim, f32_math;
};

__device__ __forceinline__ int lanes_below(unsigned long long m)
{
    return __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
}

__device__ __forceinline__ int valid_rows(const CropArgs &a)
{
    const int n = *a.n_in;
    return n < 0 ? 0 : (n > a.cap_in ? a.cap_in : n);
}

// row i of the cloud as far as the test needs it (VEC4: the whole 16-byte row, kept for the copy)
template <bool VEC4>
__device__ __forceinline__ float4 load_xyz(const CropArgs &a, int i)
{
    if (VEC4) return reinterpret_cast<const float4 *>(a.pts)[i];
    const float *p = a.pts + (size_t)i * a.ndim;
    return make_float4(p[0], p[1], p[2], 0.f);
}

template <bool VEC4>
__global__ void __launch_bounds__(kThreads) crop_count_kernel(CropArgs a)
{
    double pl[24];                                    // wave-uniform: 24 scalar loads, once
#pragma unroll
    for (int k = 0; k < 24; ++k) pl[k] = a.planes[k];
    const int n = valid_rows(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int kept = 0;
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
        const int i = blockIdx.x * kBlock + p * kThreads + threadIdx.x;
        bool keep = false;
        if (i < n) {
            const float4 v = load_xyz<VEC4>(a, i);
            keep = inside_polytope(v.x, v.y, v.z, pl, a.f32_math != 0);
        }
        kept += __popcll(__ballot(keep));
    }
    if (lane == 0) a.counts[blockIdx.x * kWaves + wave] = kept;      // rewritten in full on every call
}

template <bool VEC4>
__global__ void __launch_bounds__(kThreads) crop_scatter_kernel(CropArgs a)
{
    __shared__ int s_before[kWaves];                  // partial sums of the counts of the blocks before this one
    __shared__ int s_cnt[kPasses * kWaves];           // kept rows per (pass, wave) of this block
    double pl[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) pl[k] = a.planes[k];
    const int n_raw = *a.n_in;
    const int n = valid_rows(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    int part = 0;
    for (int k = threadIdx.x; k < (int)blockIdx.x * kWaves; k += kThreads) part += a.counts[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, 64);
    if (lane == 0) s_before[wave] = part;

    float4 row[kPasses];
    unsigned long long mask[kPasses];
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
        const int i = blockIdx.x * kBlock + p * kThreads + threadIdx.x;
        bool keep = false;
        row[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < n) {
            row[p] = load_xyz<VEC4>(a, i);
            keep = inside_polytope(row[p].x, row[p].y, row[p].z, pl, a.f32_math != 0);
        }
        mask[p] = __ballot(keep);
        if (lane == 0) s_cnt[p * kWaves + wave] = __popcll(mask[p]);
    }
    __syncthreads();

    int base = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) base += s_before[w];
    int at = base;                                    // first output row of (pass, wave) in ascending input order
#pragma unroll
    for (int p = 0; p < kPasses; ++p) {
        int mine = at;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            if (w < wave) mine += s_cnt[p * kWaves + w];
            at += s_cnt[p * kWaves + w];
        }
        const int r = mine + lanes_below(mask[p]);
        if (((mask[p] >> lane) & 1ull) && r < a.cap_out) {
            if (VEC4) {
                reinterpret_cast<float4 *>(a.out)[r] = row[p];
            } else {
                const int i = blockIdx.x * kBlock + p * kThreads + threadIdx.x;
                const uint32_t *src = reinterpret_cast<const uint32_t *>(a.pts) + (size_t)i * a.ndim;
                uint32_t *dst = reinterpret_cast<uint32_t *>(a.out) + (size_t)r * a.ndim;
                for (int c = 0; c < a.ndim; ++c) dst[c] = src[c];
            }
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {           // `at` is now the number of kept rows
        *a.n_out = at < a.cap_out ? at : a.cap_out;
        if (at > a.cap_out || n_raw > a.cap_in) atomicOr(a.status, SASSD_ST_POINT_OVERFLOW);
    }
}

inline int crop_blocks(int cap_in) { return cap_in > 0 ? cdiv(cap_in, kBlock) : 1; }
}  // namespace

extern "C" size_t sassd_crop_polytope_workspace_bytes(int cap_in)
{
    return align_up((size_t)crop_blocks(cap_in) * kWaves * sizeof(int32_t), 256);
}

extern "C" int sassd_crop_polytope_dev(const float *points, int cap_in, const int32_t *n_in_dev, int ndim,
                                       const double *planes, int f32_math, float *out, int cap_out, int32_t *n_out_dev,
                                       int32_t *status, void *ws, size_t ws_bytes, void *stream_)
{
    if (!points || !n_in_dev || !planes || !out || !n_out_dev || !status || !ws) return SASSD_EINVAL;
    if (ndim < 3 || cap_in < 0 || cap_out < 1) return SASSD_EINVAL;
    if (cap_in > INT32_MAX - kBlock) return SASSD_EINVAL;            // row indices are int32
    if (((uintptr_t)planes & 7) || ((uintptr_t)ws & 3) || (((uintptr_t)points | (uintptr_t)out) & 3)) return SASSD_EINVAL;
    if (ws_bytes < sassd_crop_polytope_workspace_bytes(cap_in)) return SASSD_EINVAL;
    CropArgs a;
    a.pts = points; a.n_in = n_in_dev; a.planes = planes; a.out = out;
    a.n_out = n_out_dev; a.status = status; a.counts = (int32_t *)ws;
    a.cap_in = cap_in; a.cap_out = cap_out; a.ndim = ndim; a.f32_math = f32_math;
    const dim3 grid(crop_blocks(cap_in)), block(kThreads);
    hipStream_t s = (hipStream_t)stream_;
    if (ndim == 4 && ((((uintptr_t)points | (uintptr_t)out) & 15) == 0)) {        // 16-byte row loads and stores
        hipLaunchKernelGGL(crop_count_kernel<true>, grid, block, 0, s, a);
        hipLaunchKernelGGL(crop_scatter_kernel<true>, grid, block, 0, s, a);
    } else {
        hipLaunchKernelGGL(crop_count_kernel<false>, grid, block, 0, s, a);
        hipLaunchKernelGGL(crop_scatter_kernel<false>, grid, block, 0, s, a);
    }
    return sassd_launch_status();
}
