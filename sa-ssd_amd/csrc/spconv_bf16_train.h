// spconv_bf16_train.h -- bf16 sparse convs for TRAINING (set_sparse_precision("bf16") / train_cfg['sparse_precision']).  Included by
// spconv.hip inside its namespace, after spconv_bf16.h and the fp32 weight-gradient kernels.
//
// Arithmetic contract: include/sassd.h "bf16 sparse backbone, training".  Every tensor a sparse kernel GATHERS is bf16 in HBM
// (the forward operand x, the gradient dy of the raw conv output); what is read contiguously or feeds statistics stays fp32 (the
// raw conv output, dx, dw).  Products of two bf16 values are exact in fp32, accumulation is fp32, no float atomics anywhere.
//
//   spconv_raw16_kernel       forward and data gradient: the rows of spconv_bf16_kernel (spconv_bf16.h: balanced work distribution,
//                             v_mfma_f32_4x4x4_16b_bf16 broadcast tiles, wave slabs summed in wave order) with the fp32 accumulator
//                             stored as it is.  The data gradient is this kernel on the forward table with the offset-reversed image
//                             of W[k]^T (submanifold) or on the transposed table with the image of W[k]^T.
//   spconv_wgrad16_kernel     weight gradient, the offset-per-wave formulation of spconv_wgrad_offset_kernel: a wave compacts the
//                             pairs of its offsets, then runs dense v_mfma_f32_16x16x16_bf16 steps with the PAIRS on the MFMA K
//                             dimension (16 pairs per instruction).  Partial sums in the [chunk][offset][Cin][Cout] layout, reduced in
//                             fixed order by wgrad_reduce_kernel.

template <int CIN, int COUT, int NW, int WPS>
__global__ void __launch_bounds__(NW * 64, WPS)
spconv_raw16_kernel(const unsigned short *__restrict__ x, const int32_t *__restrict__ nbr, const int32_t *__restrict__ n_ptr,
                    int cap, const unsigned short *__restrict__ wp, float *__restrict__ y)
{
    spconv_bf16_rows<CIN, COUT, NW, true>(x, nbr, n_ptr, cap, wp, nullptr, nullptr, 0, y);
}

template <int CIN, int COUT>
int launch_raw16(const unsigned short *x, const int32_t *nbr, const int32_t *n_ptr, int cap, const unsigned short *wp, float *y,
                 hipStream_t stream)
{
    constexpr int NW = 4, WPS = 2;
    constexpr size_t lds = gb_lds_bytes<COUT, NW>();
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    static std::atomic<unsigned long long> attr_done{0};
    const void *fn = (const void *)spconv_raw16_kernel<CIN, COUT, NW, WPS>;
    int rc = sassd_dyn_lds(fn, lds, attr_done);
    if (rc) return rc;
    hipLaunchKernelGGL((spconv_raw16_kernel<CIN, COUT, NW, WPS>), dim3(gq_grid(cap, 1)), dim3(NW * 64), lds, stream, x, nbr, n_ptr,
                       cap, wp, y);
    return sassd_launch_status();
}

// N consecutive bf16 of a row (N = 1, 2, 4: one 2 / 4 / 8-byte load)
template <int N>
__device__ __forceinline__ void load_bf16s(const unsigned short *__restrict__ p, unsigned short (&v)[N])
{
    static_assert(N == 1 || N == 2 || N == 4, "16 / 32 / 64 channels");
    if constexpr (N == 1) {
        v[0] = *p;
    } else if constexpr (N == 2) {
        const unsigned u = *(const unsigned *)p;
        v[0] = (unsigned short)(u & 0xFFFFu); v[1] = (unsigned short)(u >> 16);
    } else {
        const uint2 u = *(const uint2 *)p;
        v[0] = (unsigned short)(u.x & 0xFFFFu); v[1] = (unsigned short)(u.x >> 16);
        v[2] = (unsigned short)(u.y & 0xFFFFu); v[3] = (unsigned short)(u.y >> 16);
    }
}

// One MFMA step = 16 pairs: D[ci][co] += sum_p X[in_p][ci] * dY[out_p][co] with p on the K dimension.  Lane (m16 = lane & 15,
// q = lane >> 4) supplies K elements 4q .. 4q+3, i.e. four PAIRS, for one M row (A) and one N column (B).  The M row m16 of tile
// mt is input channel m16 * MT + mt (N column: output channel m16 * NTT + nt), so what a lane needs of one pair's row is MT
// (NTT) CONSECUTIVE bf16 and the 16 lanes of a quarter read one contiguous 32 / 64 / 128-byte segment of it.  A pair count that
// is not a multiple of 16 is padded with zeros in registers (the padded slots load row 0 of x / dy, which exists, and drop it).
template <int CIN, int COUT>
__global__ void __launch_bounds__(512) spconv_wgrad16_kernel(const unsigned short *__restrict__ x,
                                                              const unsigned short *__restrict__ dy,
                                                              const int32_t *__restrict__ nbr, const int32_t *__restrict__ n_ptr,
                                                              int cap, float *__restrict__ part, int wg_rows)
{
    static_assert(CIN % 16 == 0 && COUT % 16 == 0, "whole 16-channel MFMA tiles");
    constexpr int MT = CIN / 16, NTT = COUT / 16;
    extern __shared__ int wg_lists[];                            // [8 waves][2][wg_rows]
    const int n = min(*n_ptr, cap);
    const int r0 = blockIdx.x * wg_rows;
    if (r0 >= n) return;                                        // workgroup-uniform
    const int rows = min(wg_rows, n - r0);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = lane >> 4, m16 = lane & 15;
    int *lin = wg_lists + wave * 2 * wg_rows, *lout = lin + wg_rows;
    float *dst = part + (size_t)blockIdx.x * kK * CIN * COUT;
    // offsets of this wave: wave 0 -> 13; wave w >= 1 -> the (w-1)-th, (w+6)-th, ... of the other 26 (spconv_wgrad_offset_kernel)
#pragma unroll 1
    for (int t = 0; t < (wave == 0 ? 1 : 4); ++t) {
        int k;
        if (wave == 0) {
            k = 13;
        } else {
            const int j = (wave - 1) + 7 * t;
            if (j >= 26) break;
            k = j < 13 ? j : j + 1;
        }
        // ---- compact the (in, out) pairs of offset k over the chunk's rows (ascending row order: deterministic)
        int cnt = 0;
        for (int rb = 0; rb < rows; rb += 64) {
            const int rl = rb + lane;
            const int in = rl < rows ? nbr[(size_t)(r0 + rl) * kK + k] : -1;
            const unsigned long long m = __ballot(in >= 0);
            if (in >= 0) {
                const int pos = cnt + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
                lin[pos] = in;
                lout[pos] = r0 + rl;
            }
            cnt += __popcll(m);
        }
        __builtin_amdgcn_wave_barrier();
        f32x4 acc[MT][NTT];
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int b = 0; b < NTT; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
        s16x4 av[2][MT], bv[2][NTT];
        auto fetch = [&](int s, s16x4 *a, s16x4 *b) {
            unsigned short xa[4][MT], ya[4][NTT];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int pidx = 16 * s + 4 * q + j;            // < wg_rows: the lists hold a multiple of 64 entries
                const bool ok = pidx < cnt;
                const int in = ok ? lin[pidx] : 0, out = ok ? lout[pidx] : 0;
                load_bf16s<MT>(x + (size_t)in * CIN + m16 * MT, xa[j]);
                load_bf16s<NTT>(dy + (size_t)out * COUT + m16 * NTT, ya[j]);
#pragma unroll
                for (int i = 0; i < MT; ++i) xa[j][i] = ok ? xa[j][i] : (unsigned short)0;
#pragma unroll
                for (int i = 0; i < NTT; ++i) ya[j][i] = ok ? ya[j][i] : (unsigned short)0;
            }
#pragma unroll
            for (int i = 0; i < MT; ++i) a[i] = (s16x4){(short)xa[0][i], (short)xa[1][i], (short)xa[2][i], (short)xa[3][i]};
#pragma unroll
            for (int i = 0; i < NTT; ++i) b[i] = (s16x4){(short)ya[0][i], (short)ya[1][i], (short)ya[2][i], (short)ya[3][i]};
        };
        const int nsteps = (cnt + 15) >> 4;
        // the look-ahead fetch is unconditional -- past the end the last step is requested again (spconv_wgrad_offset_kernel)
        if (nsteps > 0) {
            fetch(0, av[0], bv[0]);
#pragma unroll 1
            for (int s = 0; s < nsteps; s += 2) {
                fetch(min(s + 1, nsteps - 1), av[1], bv[1]);
#pragma unroll
                for (int a = 0; a < MT; ++a)
#pragma unroll
                    for (int b = 0; b < NTT; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(av[0][a], bv[0][b], acc[a][b], 0, 0, 0);
                if (s + 1 >= nsteps) break;
                fetch(min(s + 2, nsteps - 1), av[0], bv[0]);
#pragma unroll
                for (int a = 0; a < MT; ++a)
#pragma unroll
                    for (int b = 0; b < NTT; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(av[1][a], bv[1][b], acc[a][b], 0, 0, 0);
            }
        }
        // D[row = q*4 + reg][col = m16] -> dW[k][ci = (q*4 + reg) * MT + a][co = m16 * NTT + b]
#pragma unroll
        for (int a = 0; a < MT; ++a)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int ci = (q * 4 + reg) * MT + a;
                float *row = dst + ((size_t)k * CIN + ci) * COUT + m16 * NTT;
#pragma unroll
                for (int b = 0; b < NTT; ++b) row[b] = acc[a][b][reg];
            }
        __builtin_amdgcn_wave_barrier();                       // the lists are rewritten for the next offset
    }
}

template <int CIN, int COUT>
int launch_wgrad16(const unsigned short *x, const unsigned short *dy, const int32_t *nbr, const int32_t *n_ptr, int cap,
                   float *part, float *dw, int accumulate, hipStream_t stream)
{
    // rows per workgroup, list size and the LDS opt-in: those of launch_wgrad (the partials have its layout)
    const int wg_rows = wgrad_rows_per_wg(cap);
    const size_t lds = (size_t)8 * 2 * wg_rows * sizeof(int);
    static std::atomic<unsigned long long> attr_done{0};
    static std::atomic<unsigned long long> attr_refused{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return SASSD_EHIP;
    const unsigned long long dbit = 1ull << (dev & 63);
    int rc = SASSD_EHIP;
    if (!(attr_refused.load(std::memory_order_acquire) & dbit)) {
        rc = sassd_dyn_lds((const void *)spconv_wgrad16_kernel<CIN, COUT>, (size_t)8 * 2 * 2048 * sizeof(int), attr_done);
        if (rc) {
            (void)hipGetLastError();
            attr_refused.fetch_or(dbit, std::memory_order_release);
        }
    }
    if (rc && lds > 64 * 1024) return rc;
    hipLaunchKernelGGL((spconv_wgrad16_kernel<CIN, COUT>), dim3(cdiv(cap, wg_rows)), dim3(512), lds, stream, x, dy, nbr, n_ptr,
                       cap, part, wg_rows);
    const int per = kK * CIN * COUT;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(cdiv(per, 32)), dim3(256), 0, stream, (const float *)part, n_ptr, cap, per, dw,
                       accumulate, wg_rows);
    return sassd_launch_status();
}
