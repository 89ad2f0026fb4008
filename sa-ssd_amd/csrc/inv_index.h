// inv_index.h -- ordered scatter-to-gather of 3-NN interpolation gradients (the deterministic training mode, sassd.h
// "Deterministic training").  Shared by aux_head.hip (three levels) and pointops.hip (sassd_three_interpolate_grad_det).
//
// An inverted index of the [n, 3] neighbour lists of up to three levels: for every destination row (rows of all levels
// concatenated), the entries e = level * 3n + p * 3 + j with idx_level[p, j] == row, in ASCENDING e.  Four launches:
//   inv_zero_kernel    counts = 0                                 (plain stores: no hipMemsetAsync, capture-safe)
//   inv_count_kernel   counts[row] += 1 per entry                 (integer atomics: a list length, order-free)
//   inv_scan_kernel    start[row] = exclusive prefix sum, cursor = start   (one workgroup, fixed order)
//   inv_fill_kernel    unsorted[cursor[row]++] = e                (integer atomic cursor: ARBITRARY order in a segment)
//   inv_rank_kernel    sorted[start[row] + #{e' in segment : e' < e}] = e   (the segment sorted by rank counting: the
//                      atomic placement never reaches a float sum)
// Entries whose index lies outside [0, M_level) are left out (the atomic kernels would write out of bounds).
// The gather pass (one thread per (row, channel)) then sums the rounded products in list order; it lives next to its
// callers because the gradient / weight layouts differ.
#pragma once
#include "common.h"

namespace {
struct InvIndex {
    const int32_t *idx[3];          // [n, 3] per level
    int M[3];                       // rows per level
    int row0[3];                    // first global row of each level
    int levels, n, rows;            // rows = M[0] + .. + M[levels - 1]
    int *count;                     // [rows]
    int *start;                     // [rows + 1]
    int *cursor;                    // [rows]
    int *unsorted;                  // [levels * 3n]
    int *sorted;                    // [levels * 3n]
};

// global row of entry e, or -1 (out of range)
__device__ __forceinline__ int inv_row(const InvIndex &X, int e)
{
    const int per = 3 * X.n;
    const int s = e / per;
    const int r = X.idx[s][e - s * per];
    return (r >= 0 && r < X.M[s]) ? X.row0[s] + r : -1;
}

__global__ void __launch_bounds__(256) inv_zero_kernel(InvIndex X)
{
    for (int i = blockIdx.x * 256 + threadIdx.x; i < X.rows; i += gridDim.x * 256) X.count[i] = 0;
}

__global__ void __launch_bounds__(256) inv_count_kernel(InvIndex X)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= X.levels * 3 * X.n) return;
    const int r = inv_row(X, e);
    if (r >= 0) atomicAdd(X.count + r, 1);
}

// one workgroup of 1024: each thread owns a contiguous run of rows (sum, block scan of the run sums, re-read and write)
__global__ void __launch_bounds__(1024) inv_scan_kernel(InvIndex X)
{
    __shared__ int wsum[16];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int per = (X.rows + 1023) / 1024;
    const int lo = min(t * per, X.rows), hi = min(lo + per, X.rows);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += X.count[i];
    // inclusive scan of s over the workgroup
    int v = s;
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    if (lane == 63) wsum[wv] = v;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wv; ++w) base += wsum[w];
    int run = base + v - s;                                      // exclusive prefix of this thread's run
    for (int i = lo; i < hi; ++i) {
        X.start[i] = run;
        X.cursor[i] = run;
        run += X.count[i];
    }
    if (t == 1023) X.start[X.rows] = base + v;
}

__global__ void __launch_bounds__(256) inv_fill_kernel(InvIndex X)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= X.levels * 3 * X.n) return;
    const int r = inv_row(X, e);
    if (r >= 0) X.unsorted[atomicAdd(X.cursor + r, 1)] = e;
}

// one thread per list position: its rank among the entries of its segment is its place in the sorted list
__global__ void __launch_bounds__(256) inv_rank_kernel(InvIndex X)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= X.start[X.rows]) return;
    const int e = X.unsorted[i];
    const int r = inv_row(X, e);
    const int lo = X.start[r], hi = X.start[r + 1];
    int rank = 0;
    for (int k = lo; k < hi; ++k) rank += X.unsorted[k] < e ? 1 : 0;
    X.sorted[lo + rank] = e;
}

// workspace: count [rows], start [rows + 1], cursor [rows], unsorted / sorted [levels * 3n] int32, 256-byte aligned
inline size_t inv_index_bytes(int levels, int n, long rows)
{
    const size_t e = (size_t)levels * 3 * (size_t)n;
    return align_up((size_t)rows * 4, 256) * 2 + align_up(((size_t)rows + 1) * 4, 256) + align_up(e * 4, 256) * 2;
}

inline void inv_index_carve(InvIndex &X, void *ws)
{
    char *w = (char *)ws;
    const size_t e = (size_t)X.levels * 3 * (size_t)X.n;
    X.count = (int *)w;      w += align_up((size_t)X.rows * 4, 256);
    X.cursor = (int *)w;     w += align_up((size_t)X.rows * 4, 256);
    X.start = (int *)w;      w += align_up(((size_t)X.rows + 1) * 4, 256);
    X.unsorted = (int *)w;   w += align_up(e * 4, 256);
    X.sorted = (int *)w;
}

inline void inv_index_build(const InvIndex &X, hipStream_t s)
{
    const int ne = X.levels * 3 * X.n;
    const int zb = X.rows > 0 ? (cdiv(X.rows, 256) < 1024 ? cdiv(X.rows, 256) : 1024) : 1;
    hipLaunchKernelGGL(inv_zero_kernel, dim3(zb), dim3(256), 0, s, X);
    if (ne > 0) hipLaunchKernelGGL(inv_count_kernel, dim3(cdiv(ne, 256)), dim3(256), 0, s, X);
    hipLaunchKernelGGL(inv_scan_kernel, dim3(1), dim3(1024), 0, s, X);
    if (ne > 0) {
        hipLaunchKernelGGL(inv_fill_kernel, dim3(cdiv(ne, 256)), dim3(256), 0, s, X);
        hipLaunchKernelGGL(inv_rank_kernel, dim3(cdiv(ne, 256)), dim3(256), 0, s, X);
    }
}
}  // namespace
