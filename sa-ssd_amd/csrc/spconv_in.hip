// spconv_in.hip -- the sparse INPUT layer SubMConv3d(Cin, 16, 3) for 3 <= Cin <= 8 features per voxel (the per-voxel means
// of clouds that carry more, or fewer, than KITTI's x, y, z, intensity: elongation, a sweep's time offset, painted class
// scores).  Contract in include/sassd.h, "Sparse input layer".  spconv.hip keeps the 4-channel layer it always ran
// (spconv_c4_kernel, spconv_gq.h); Cin = 4 is instantiated here as well so that the tests can hold these kernels to that
// one bit for bit -- no caller is dispatched to it.
//
// Forward: the design of spconv_c4_kernel.  27 * Cin multiply-adds per output value are nothing for a matrix core: 16
// consecutive threads own one output row (one output channel each), the row's rulebook record and its neighbours' feature
// rows are read once per 16 threads (the same address in all of them: one request), the weights sit in LDS, k ascending and
// channels ascending within k -- one fmaf chain, a fixed summation order.  Latency is hidden by occupancy.
//   feature rows   [rows][Cin], row stride Cin floats, as the voxelizer writes them: 12 to 32 bytes, so a row is only as
//                  aligned as Cin * 4 is (16 bytes for Cin 4 and 8, 8 for Cin 6, 4 for the odd widths); the loads are the
//                  widest that alignment allows.  The features are never padded; the weight image is.
//   weight image   [27][CP/4][16][4] with CP = Cin rounded up to a multiple of 4 and zeros in the padding: element
//                  (k, c, co) at ((k * CP/4 + c/4) * 16 + co) * 4 + c % 4, i.e. the threads of a row read consecutive 16-byte
//                  LDS pieces.  At Cin = 4 this IS the image of sassd_spconv_pack_weight.  The padding is never multiplied.
// Weight gradient: thread (k, co) of a 448-thread workgroup keeps dw[k][0..Cin-1][co] in registers and walks the rows of its
// chunk in ascending order (rulebook records and dy rows staged in LDS 128 rows at a time, the gathered x rows straight from
// L2); every workgroup leaves one [27][Cin][16] partial in the caller's workspace and a second kernel adds the partials in a
// fixed order: no atomics, two calls agree bit for bit.
#include "common.h"

#include <type_traits>

namespace {

constexpr int kK = 27, kCout = 16;
constexpr int kStage = 128;        // rows of rulebook + dy staged per step of the weight gradient

constexpr int in_cp(int cin) { return (cin + 3) / 4 * 4; }

static inline bool in_shape(int K, int Cin, int Cout) { return K == kK && Cin >= 3 && Cin <= 8 && Cout == kCout; }

// rows per weight-gradient workgroup: 128 up to 64 k rows, then capacity / 512 (a multiple of 128, <= 2048), so that the
// partials stay at <= ~512 per call
static inline int in_wg_rows(int cap)
{
    int r = ((cap + 511) / 512 + kStage - 1) / kStage * kStage;
    return r < kStage ? kStage : (r > 2048 ? 2048 : r);
}

// one feature row in the widest pieces its alignment allows (x itself is 16-byte aligned: checked by the entry points)
template <int CIN>
__device__ __forceinline__ void load_row(const float *__restrict__ p, float (&v)[CIN])
{
    if constexpr (CIN % 4 == 0) {
#pragma unroll
        for (int i = 0; i < CIN / 4; ++i) {
            const float4 t = ((const float4 *)p)[i];
            v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
        }
    } else if constexpr (CIN % 2 == 0) {
#pragma unroll
        for (int i = 0; i < CIN / 2; ++i) {
            const float2 t = ((const float2 *)p)[i];
            v[2 * i] = t.x; v[2 * i + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < CIN; ++i) v[i] = p[i];
    }
}

template <int CIN>
__global__ void pack_in_kernel(const float *__restrict__ w, float *__restrict__ packed)
{
    constexpr int CP = in_cp(CIN);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= kK * CP * kCout) return;
    const int r = i & 3;
    const int co = (i >> 2) % kCout;
    const int c4 = (i / (4 * kCout)) % (CP / 4);
    const int k = i / (CP * kCout);
    const int ci = c4 * 4 + r;
    packed[i] = ci < CIN ? w[((size_t)k * CIN + ci) * kCout + co] : 0.f;
}

template <int CIN, typename TY>
__global__ void __launch_bounds__(256)
spconv_in_kernel(const float *__restrict__ x, const int32_t *__restrict__ nbr, const int32_t *__restrict__ n_ptr, int cap,
                 const float *__restrict__ wp, const float *__restrict__ scale, const float *__restrict__ shift, int relu,
                 TY *__restrict__ y)
{
    constexpr int C4 = in_cp(CIN) / 4;
    __shared__ float4 ws[kK * C4 * kCout];
    for (int i = threadIdx.x; i < kK * C4 * kCout; i += 256) ws[i] = ((const float4 *)wp)[i];
    __syncthreads();
    const int n = min(*n_ptr, cap);
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int row = t / kCout, co = t - row * kCout;
    if (row >= n) return;
    const int32_t *nb = nbr + (size_t)row * kK;
    float acc = 0.f;
#pragma unroll 9
    for (int k = 0; k < kK; ++k) {
        const int in = nb[k];
        if (in >= 0) {
            float xv[CIN];
            load_row<CIN>(x + (size_t)in * CIN, xv);
            float wf[4 * C4];
#pragma unroll
            for (int c4 = 0; c4 < C4; ++c4) {
                const float4 wv = ws[(k * C4 + c4) * kCout + co];
                wf[4 * c4] = wv.x; wf[4 * c4 + 1] = wv.y; wf[4 * c4 + 2] = wv.z; wf[4 * c4 + 3] = wv.w;
            }
#pragma unroll
            for (int c = 0; c < CIN; ++c) acc = fmaf(xv[c], wf[c], acc);     // channels ascending; the padding is not touched
        }
    }
    float o = acc * (scale ? scale[co] : 1.f) + (shift ? shift[co] : 0.f);
    if (relu) o = fmaxf(o, 0.f);
    if constexpr (std::is_same<TY, float>::value) y[(size_t)row * kCout + co] = o;
    else y[(size_t)row * kCout + co] = __builtin_bit_cast(unsigned short, (__bf16)o);
}

template <int CIN>
int launch_in(const float *x, const int32_t *nbr, const int32_t *n_ptr, int cap, const float *wp, const float *scale,
              const float *shift, int relu, void *y, int y_bf16, hipStream_t stream)
{
    const dim3 grid(cdiv(cap, 256 / kCout));
    if (y_bf16)
        hipLaunchKernelGGL((spconv_in_kernel<CIN, unsigned short>), grid, dim3(256), 0, stream, x, nbr, n_ptr, cap, wp, scale,
                           shift, relu, (unsigned short *)y);
    else
        hipLaunchKernelGGL((spconv_in_kernel<CIN, float>), grid, dim3(256), 0, stream, x, nbr, n_ptr, cap, wp, scale, shift,
                           relu, (float *)y);
    return sassd_launch_status();
}

template <int CIN>
int launch_pack_in(const float *w, float *packed, hipStream_t stream)
{
    hipLaunchKernelGGL((pack_in_kernel<CIN>), dim3(cdiv(kK * in_cp(CIN) * kCout, 256)), dim3(256), 0, stream, w, packed);
    return sassd_launch_status();
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------
constexpr int kWgThreads = 448;    // 27 offsets x 16 output channels = 432 accumulating threads in 7 waves

template <int CIN>
__global__ void __launch_bounds__(kWgThreads)
spconv_in_wgrad_kernel(const float *__restrict__ x, const float *__restrict__ dy, const int32_t *__restrict__ nbr,
                       const int32_t *__restrict__ n_ptr, int cap, float *__restrict__ part, int wg_rows)
{
    __shared__ int nbr_s[kStage * kK];
    __shared__ float dy_s[kStage * kCout];
    const int n = min(*n_ptr, cap);
    const int r0 = blockIdx.x * wg_rows;
    if (r0 >= n) return;                                        // workgroup-uniform; the reduce kernel skips this partial
    const int rows = min(wg_rows, n - r0);
    const int tid = threadIdx.x;
    const int k = tid >> 4, co = tid & 15;
    float acc[CIN];
#pragma unroll
    for (int c = 0; c < CIN; ++c) acc[c] = 0.f;
    for (int s0 = 0; s0 < rows; s0 += kStage) {
        const int sr = min(kStage, rows - s0);
        if (s0) __syncthreads();                                // the previous step's reads are done
        for (int i = tid; i < sr * kK; i += kWgThreads) nbr_s[i] = nbr[(size_t)(r0 + s0) * kK + i];
        for (int i = tid; i < sr * kCout; i += kWgThreads) dy_s[i] = dy[(size_t)(r0 + s0) * kCout + i];
        __syncthreads();
        if (k < kK) {
#pragma unroll 4
            for (int r = 0; r < sr; ++r) {                      // ascending rows: the summation order
                const int in = nbr_s[r * kK + k];
                if (in >= 0) {
                    float xv[CIN];
                    load_row<CIN>(x + (size_t)in * CIN, xv);
                    const float d = dy_s[r * kCout + co];
#pragma unroll
                    for (int c = 0; c < CIN; ++c) acc[c] = fmaf(xv[c], d, acc[c]);
                }
            }
        }
    }
    if (k < kK) {
        float *dst = part + (size_t)blockIdx.x * kK * CIN * kCout;
#pragma unroll
        for (int c = 0; c < CIN; ++c) dst[((size_t)k * CIN + c) * kCout + co] = acc[c];
    }
}

// dw = sum of the per-workgroup partials in a fixed order: 8 threads per element take every 8th partial (two accumulators
// each), the eight sums meet in LDS (the scheme of wgrad_reduce_kernel in spconv.hip)
__global__ void __launch_bounds__(256) spconv_in_wgrad_reduce_kernel(const float *__restrict__ part,
                                                                     const int32_t *__restrict__ n_ptr, int cap, int per,
                                                                     float *__restrict__ dw, int accumulate, int wg_rows)
{
    __shared__ float red[8][32];
    const int n = min(*n_ptr, cap);
    const int nwg = (n + wg_rows - 1) / wg_rows;
    const int e = threadIdx.x & 31, pt = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + e;
    float s0 = 0.f, s1 = 0.f;
    if (i < per) {
        int g = pt;
        for (; g + 8 < nwg; g += 16) {
            s0 += part[(size_t)g * per + i];
            s1 += part[(size_t)(g + 8) * per + i];
        }
        if (g < nwg) s0 += part[(size_t)g * per + i];
    }
    red[pt][e] = s0 + s1;
    __syncthreads();
    if (pt == 0 && i < per) {
        float s = accumulate ? dw[i] : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) s += red[j][e];
        dw[i] = s;
    }
}

template <int CIN>
int launch_wgrad_in(const float *x, const float *dy, const int32_t *nbr, const int32_t *n_ptr, int cap, float *part, float *dw,
                    int accumulate, hipStream_t stream)
{
    const int wg_rows = in_wg_rows(cap);
    hipLaunchKernelGGL((spconv_in_wgrad_kernel<CIN>), dim3(cdiv(cap, wg_rows)), dim3(kWgThreads), 0, stream, x, dy, nbr, n_ptr,
                       cap, part, wg_rows);
    const int per = kK * CIN * kCout;
    hipLaunchKernelGGL(spconv_in_wgrad_reduce_kernel, dim3(cdiv(per, 32)), dim3(256), 0, stream, (const float *)part, n_ptr,
                       cap, per, dw, accumulate, wg_rows);
    return sassd_launch_status();
}

#define IN_DISPATCH(FN, ...)                          \
    switch (Cin) {                                    \
    case 3: return FN<3>(__VA_ARGS__);                \
    case 4: return FN<4>(__VA_ARGS__);                \
    case 5: return FN<5>(__VA_ARGS__);                \
    case 6: return FN<6>(__VA_ARGS__);                \
    case 7: return FN<7>(__VA_ARGS__);                \
    case 8: return FN<8>(__VA_ARGS__);                \
    default: return SASSD_EINVAL;                     \
    }

}  // namespace

extern "C" int sassd_spconv_in_supported(int K, int Cin, int Cout) { return in_shape(K, Cin, Cout) ? 1 : 0; }

extern "C" size_t sassd_spconv_in_packed_floats(int K, int Cin, int Cout)
{
    return in_shape(K, Cin, Cout) ? (size_t)kK * in_cp(Cin) * kCout : 0;
}

extern "C" int sassd_spconv_in_pack_weight(const float *w, int K, int Cin, int Cout, float *packed, void *stream_)
{
    if (!w || !packed || !in_shape(K, Cin, Cout)) return SASSD_EINVAL;
    if ((uintptr_t)packed & 15) return SASSD_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    IN_DISPATCH(launch_pack_in, w, packed, stream)
}

extern "C" int sassd_spconv_in_fwd(const float *x, const int32_t *nbr, const int32_t *n_out_ptr, int cap_out,
                                   const float *w_packed, int K, int Cin, int Cout, const float *scale, const float *shift,
                                   int relu, void *y, int y_bf16, void *stream_)
{
    if (!x || !nbr || !n_out_ptr || !w_packed || !y || cap_out <= 0 || !in_shape(K, Cin, Cout)) return SASSD_EINVAL;
    if ((cap_out + 15) / 16 > 0x7FFFFFF) return SASSD_EINVAL;                 // 16 threads per row: the grid stays in 31 bits
    if (((uintptr_t)x | (uintptr_t)w_packed) & 15) return SASSD_EINVAL;      // rows are loaded in pieces of up to 16 bytes
    if ((uintptr_t)y & (y_bf16 ? 1 : 3)) return SASSD_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    const int r = relu ? 1 : 0, b = y_bf16 ? 1 : 0;
    IN_DISPATCH(launch_in, x, nbr, n_out_ptr, cap_out, w_packed, scale, shift, r, y, b, stream)
}

extern "C" size_t sassd_spconv_in_bwd_weight_workspace_bytes(int cap_out, int K, int Cin, int Cout)
{
    if (!in_shape(K, Cin, Cout) || cap_out <= 0) return 0;
    return (size_t)cdiv(cap_out, in_wg_rows(cap_out)) * kK * Cin * kCout * sizeof(float);
}

extern "C" int sassd_spconv_in_bwd_weight(const float *x, const float *dy, const int32_t *nbr, const int32_t *n_out_ptr,
                                          int cap_out, int K, int Cin, int Cout, float *dw, int accumulate, void *workspace,
                                          size_t workspace_bytes, void *stream_)
{
    if (!x || !dy || !nbr || !n_out_ptr || !dw || !workspace || cap_out <= 0 || !in_shape(K, Cin, Cout)) return SASSD_EINVAL;
    if (workspace_bytes < sassd_spconv_in_bwd_weight_workspace_bytes(cap_out, K, Cin, Cout)) return SASSD_EINVAL;
    if (((uintptr_t)x & 15) || ((uintptr_t)workspace & 3)) return SASSD_EINVAL;
    hipStream_t stream = (hipStream_t)stream_;
    IN_DISPATCH(launch_wgrad_in, x, dy, nbr, n_out_ptr, cap_out, (float *)workspace, dw, accumulate ? 1 : 0, stream)
}
