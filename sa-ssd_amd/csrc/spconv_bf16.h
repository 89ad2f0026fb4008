// spconv_bf16.h -- bf16 sparse-conv forward for inference (InferencePlan(sparse_precision="bf16")).  Included by spconv.hip
// inside its namespace, after spconv_gq.h.
//
// Arithmetic contract: include/sassd.h "bf16 sparse backbone" and DESIGN.md section 2.  In short: features are stored bf16 in
// HBM (128 B per 64-channel row instead of 256 B), the raw weights are rounded once to bf16 at pack time, every product of two
// bf16 values is exact in fp32 and accumulated in fp32, the epilogue relu(acc * scale + shift) runs in fp32 and the result is
// rounded to bf16 (nearest even) by a plain cast at the store.
//
// Work distribution: that of spconv_gq_kernel with ILV = 1 (XCD-local blocks of <= 2048 rows, 32 interleaved slices per block,
// cooperative compaction of the 27 offsets, the unit list cut into NW equal contiguous ranges, one private fp32 LDS slab per
// wave, slabs summed in wave order) -- the summation order is a function of the rulebook only, no atomics anywhere.  What
// changes is the tile: v_mfma_f32_4x4x4_16b_bf16 in the broadcast form of the fp32 quad path.  The A operand of one block
// (4 pairs x 4 input channels, one 64-bit register per lane) is broadcast to the blocks of its group (CBSZ / ABID), B = W[k][4
// input channels][one output channel per lane], so one instruction is 4 * (64 / COUT) pairs x COUT output channels x 4 input
// channels.  COUT = 16 works the same way with groups of 4 blocks (CBSZ = 2): 16 pairs per instruction.
// Weight image: [K][COUT][CIN] bf16 -- a lane's weights for one offset are CIN consecutive bf16 (CIN / 4 registers).
// nbr == nullptr is the 1x1x1 layer (identity rulebook): every row pairs with itself at the centre offset.

typedef short s16x4 __attribute__((ext_vector_type(4)));

// RAW (training, spconv_bf16_train.h): the same rows, the fp32 accumulator stored as it is -- no scale / shift / ReLU, no rounding.
template <int CIN, int COUT, int NW, bool RAW>
__device__ __forceinline__ void
spconv_bf16_rows(const unsigned short *__restrict__ x, const int32_t *__restrict__ nbr, const int32_t *__restrict__ n_ptr,
                 int cap, const unsigned short *__restrict__ wp, const float *__restrict__ scale,
                 const float *__restrict__ shift, int relu, void *__restrict__ y_)
{
    static_assert(COUT == 16 || COUT == 32 || COUT == 64, "4x4x4 broadcast tile: 16 / 32 / 64 output channels");
    static_assert(CIN % 16 == 0, "a lane's channel quarter is a whole number of 4-channel MFMA steps");
    constexpr int RW = 64, T = NW * 64;
    constexpr int KSEG = CIN / 4;                            // input channels of one quarter
    constexpr int KV = KSEG / 4;                             // 4-channel registers (MFMA steps) per quarter
    constexpr int NH2 = 64 / COUT;                           // pair quads one instruction covers (1, 2 or 4)
    constexpr int PPS = 4 * NH2;                             // pairs per instruction set
    constexpr int NS = 16 / PPS;                             // instruction sets per 16-pair tile
    constexpr int BG = 16 / NH2;                             // MFMA blocks that share one broadcast A block
    constexpr int CBSZ = (BG == 16) ? 4 : (BG == 8) ? 3 : 2;
    constexpr int UNIT = PPS;                                // pairs per unit of the balanced partition
    constexpr int UPT = 16 / UNIT;                           // units per tile
    extern __shared__ __attribute__((aligned(16))) float gb_lds[];
    float *slabs = gb_lds;                                   // [NW][RW][COUT]
    int *nbr_s = (int *)(gb_lds + NW * RW * COUT);           // [RW][27]
    int *lists = nbr_s + RW * kK;                            // [27][RW]  (input row << 6 | local output row)
    int *cnt = lists + kK * RW;                              // [27]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // ---- workgroup -> (XCD-local block, interleaved slice): spconv_gq_kernel, ILV = 1 -------------------------------------
    const int xcd = (int)(blockIdx.x & 7), t_ = (int)(blockIdx.x >> 3);
    const int n = min(*n_ptr, cap);
    const int sl = t_ & 31, j8 = t_ >> 5;
    const int nb8 = n <= 16384 ? 1 : (n + 16383) / 16384;
    if (j8 >= nb8) return;                                   // workgroup-uniform
    const int bs = (n + 8 * nb8 - 1) / (8 * nb8);            // rows per block, <= 2048
    const int base = (j8 * 8 + xcd) * bs;
    const int brows = min(bs, n - base);
    if (brows <= sl) return;
    const int rows = (brows - sl + 31) >> 5;                 // <= 64
    const int row0 = base + sl;
    constexpr int RS = 32;
    constexpr int NST = (RW * kK + T - 1) / T;
    int stage[NST];
#pragma unroll
    for (int j = 0; j < NST; ++j) {
        const int i = tid + j * T;
        const int r = i / kK, kk = i - r * kK;
        const int row = row0 + RS * r;
        stage[j] = (r < rows) ? (nbr ? nbr[(size_t)row * kK + kk] : (kk == kK / 2 ? row : -1)) : -1;
    }
    for (int i = tid; i < NW * RW * COUT / 4; i += T) ((float4 *)slabs)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < NST; ++j) {
        const int i = tid + j * T;
        if (i < RW * kK) nbr_s[i] = stage[j];
    }
    __syncthreads();
    // ---- cooperative compaction of the 27 offsets ---------------------------------------------------------------------
    for (int k = wave; k < kK; k += NW) {
        const int v = nbr_s[lane * kK + k];
        const unsigned long long mk = __ballot(v >= 0);
        const int pos = __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0));
        if (v >= 0) lists[k * RW + pos] = (v << 6) | lane;
        if (lane == 0) cnt[k] = __popcll(mk);
    }
    __syncthreads();

    // ---- balanced partition: units of UNIT pairs, offsets heaviest first, NW equal contiguous ranges ------------------
    const int k_l = c_offset_order[lane < kK ? lane : 0];
    const int c_l = (lane < kK) ? cnt[k_l] : 0;
    const int u_l = (c_l + UNIT - 1) / UNIT;
    int incl = u_l;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(incl, o, 64);
        if (lane >= o) incl += t;
    }
    const int total = __builtin_amdgcn_readlane(incl, kK - 1);
    const int lo = (int)(((long long)wave * total) / NW), hi = (int)(((long long)(wave + 1) * total) / NW);

    float *slab = slabs + wave * RW * COUT;
    // lane -> (pair of the tile, input-channel quarter): block b = lane / 4 = h * BG + a, a = G * NS + set
    const int blk = lane >> 2;
    const int a_ = blk % BG, h_ = blk / BG;
    const int G_l = a_ / NS;
    const int pl = PPS * (a_ % NS) + 4 * h_ + (lane & 3);
    const int cl = lane % COUT;                              // this lane's output channel
    const int hq = lane / COUT;                              // which quad of an instruction set this lane's D rows are

    struct Tile { int slot, k, pb, np; };
    auto locate = [&](int g, Tile &tl) -> int {
        const unsigned long long m = __ballot(incl > g);
        const int slot = __builtin_ctzll(m);
        const int cs = __builtin_amdgcn_readlane(c_l, slot), is = __builtin_amdgcn_readlane(incl, slot);
        const int us = __builtin_amdgcn_readlane(u_l, slot);
        const int uo = g - (is - us);
        const int tu = min(UPT, min(us - uo, hi - g));
        tl.slot = slot;
        tl.k = __builtin_amdgcn_readlane(k_l, slot);
        tl.pb = uo * UNIT;
        tl.np = min(tu * UNIT, cs - tl.pb);
        return tu;
    };
    auto next_slot_k = [&](int slot) -> int {
        const int is = __builtin_amdgcn_readlane(incl, slot);
        if (is >= hi) return -1;
        const unsigned long long m = __ballot(incl > is);
        return __builtin_amdgcn_readlane(k_l, __builtin_ctzll(m));
    };
    // gathered operand: KSEG consecutive bf16 of the pair's input row (channels G * KSEG ..), KV 64-bit registers
    auto fetch_a = [&](const Tile &tl, s16x4 (&af)[KV]) {
        const int e = lists[tl.k * RW + tl.pb + (pl < tl.np ? pl : 0)];
        const s16x4 *p = (const s16x4 *)(x + (size_t)(e >> 6) * CIN + G_l * KSEG);
#pragma unroll
        for (int j = 0; j < KV; ++j) af[j] = p[j];
    };
    constexpr int NB = CIN / 4;                              // weight registers of one offset: b[c4] = W[k][4 c4 .. 4 c4 + 3][cl]
    auto load_w = [&](int k, s16x4 (&b)[NB]) {
        const s16x4 *wk = (const s16x4 *)(wp + ((size_t)(nbr ? k : 0) * COUT + cl) * CIN);
#pragma unroll
        for (int j = 0; j < NB; ++j) b[j] = wk[j];
    };
    auto tile = [&](const Tile &tl, const s16x4 (&af)[KV], const s16x4 (&b)[NB]) {
        const int *lst = lists + tl.k * RW + tl.pb;
        // one instruction set = PPS pairs x COUT channels x CIN: four accumulator chains (one per input-channel quarter),
        // started from zero and added to the slab rows at the end
        auto qset = [&](auto sc) {
            constexpr int s = decltype(sc)::value;
            if constexpr (s < NS) {
                if (s * PPS < tl.np) {                              // wave-uniform
                    float *rowp[4];
                    bool ok[4];
                    float c0[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int p = s * PPS + 4 * hq + i;
                        ok[i] = p < tl.np;
                        const int e = lst[ok[i] ? p : 0];
                        rowp[i] = slab + (e & 63) * COUT + cl;
                        c0[i] = *rowp[i];
                    }
                    f32x4 d0 = (f32x4){0.f, 0.f, 0.f, 0.f}, d1 = d0, d2 = d0, d3 = d0;
#pragma unroll
                    for (int j = 0; j < KV; ++j) {
                        d0 = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(af[j], b[0 * KV + j], d0, CBSZ, 0 * NS + s, 0);
                        d1 = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(af[j], b[1 * KV + j], d1, CBSZ, 1 * NS + s, 0);
                        d2 = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(af[j], b[2 * KV + j], d2, CBSZ, 2 * NS + s, 0);
                        d3 = __builtin_amdgcn_mfma_f32_4x4x4bf16_1k(af[j], b[3 * KV + j], d3, CBSZ, 3 * NS + s, 0);
                    }
                    const f32x4 sum = (d0 + d1) + (d2 + d3);
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (ok[i]) *rowp[i] = c0[i] + sum[i];
                }
            }
        };
        qset(std::integral_constant<int, 0>{});
        qset(std::integral_constant<int, 1>{});
        qset(std::integral_constant<int, 2>{});
        qset(std::integral_constant<int, 3>{});
    };

    if (lo < hi) {
        s16x4 b0[NB], b1[NB];
        s16x4 a0[KV], a1[KV];
        Tile cur, nxt;
        int g = lo;
        g += locate(g, cur);
        fetch_a(cur, a0);
        load_w(cur.k, b0);
        // the software pipeline of spconv_gq_kernel: prefetches unconditional (past the end the current tile / offset is
        // requested again), the next offset's weights requested once the first tile of this one is issued
        auto run_slot = [&](const s16x4 (&b)[NB], s16x4 (&bn)[NB]) -> bool {
            const int slot = cur.slot;
            bool first = true;
            for (;;) {
                bool more = g < hi;
                nxt = cur;
                if (more) g += locate(g, nxt);
                fetch_a(nxt, a1);
                tile(cur, a0, b);
                if (first) {
                    const int kn = next_slot_k(slot);
                    load_w(kn >= 0 ? kn : cur.k, bn);
                    first = false;
                }
                if (!more) return false;
                cur = nxt;
                if (cur.slot != slot) {
#pragma unroll
                    for (int i = 0; i < KV; ++i) a0[i] = a1[i];
                    return true;
                }
                more = g < hi;
                nxt = cur;
                if (more) g += locate(g, nxt);
                fetch_a(nxt, a0);
                tile(cur, a1, b);
                if (!more) return false;
                cur = nxt;
                if (cur.slot != slot) return true;
            }
        };
        for (;;) {
            if (!run_slot(b0, b1)) break;
            if (!run_slot(b1, b0)) break;
        }
    }
    __syncthreads();

    // ---- epilogue: the wave slabs summed in wave order, relu(acc * scale + shift) in fp32, bf16 store (8 bytes) ---------
    constexpr int C4 = COUT / 4;
    for (int i = tid; i < rows * C4; i += T) {
        const int r = i / C4, c4 = i - r * C4;
        const float *src = slabs + r * COUT + c4 * 4;
        float4 v = *(const float4 *)src;
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            const float4 p = *(const float4 *)(src + w * RW * COUT);
            v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
        }
        if constexpr (RAW) {
            *(float4 *)((float *)y_ + (size_t)(row0 + RS * r) * COUT + c4 * 4) = v;
            continue;
        }
        unsigned short *y = (unsigned short *)y_;
        const float4 sc = scale ? *(const float4 *)(scale + c4 * 4) : make_float4(1.f, 1.f, 1.f, 1.f);
        const float4 sh = shift ? *(const float4 *)(shift + c4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
        v.x = v.x * sc.x + sh.x; v.y = v.y * sc.y + sh.y; v.z = v.z * sc.z + sh.z; v.w = v.w * sc.w + sh.w;
        if (relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
        const ushort4 o = make_ushort4(__builtin_bit_cast(unsigned short, (__bf16)v.x), __builtin_bit_cast(unsigned short, (__bf16)v.y),
                                       __builtin_bit_cast(unsigned short, (__bf16)v.z), __builtin_bit_cast(unsigned short, (__bf16)v.w));
        *(ushort4 *)(y + (size_t)(row0 + RS * r) * COUT + c4 * 4) = o;
    }
}

template <int CIN, int COUT, int NW, int WPS>
__global__ void __launch_bounds__(NW * 64, WPS)
spconv_bf16_kernel(const unsigned short *__restrict__ x, const int32_t *__restrict__ nbr, const int32_t *__restrict__ n_ptr,
                   int cap, const unsigned short *__restrict__ wp, const float *__restrict__ scale,
                   const float *__restrict__ shift, int relu, unsigned short *__restrict__ y)
{
    spconv_bf16_rows<CIN, COUT, NW, false>(x, nbr, n_ptr, cap, wp, scale, shift, relu, y);
}

template <int COUT, int NW>
constexpr size_t gb_lds_bytes() { return (size_t)(NW * 64 * COUT + 64 * kK + kK * 64 + 32) * 4; }

// grid: 256 workgroups per 16 k rows of capacity (the block / slice map above serves every capacity below 2^25 rows)
template <int CIN, int COUT>
int launch_bf16(const unsigned short *x, const int32_t *nbr, const int32_t *n_ptr, int cap, const unsigned short *wp,
                const float *scale, const float *shift, int relu, unsigned short *y, hipStream_t stream)
{
    constexpr int NW = 4, WPS = 2;
    constexpr size_t lds = gb_lds_bytes<COUT, NW>();
    static_assert(lds <= 80 * 1024, "two workgroups per CU");
    static std::atomic<unsigned long long> attr_done{0};
    const void *fn = (const void *)spconv_bf16_kernel<CIN, COUT, NW, WPS>;
    int rc = sassd_dyn_lds(fn, lds, attr_done);
    if (rc) return rc;
    hipLaunchKernelGGL((spconv_bf16_kernel<CIN, COUT, NW, WPS>), dim3(gq_grid(cap, 1)), dim3(NW * 64), lds, stream, x, nbr, n_ptr,
                       cap, wp, scale, shift, relu, y);
    return sassd_launch_status();
}

// w [K][CIN][COUT] fp32 -> [K][COUT][CIN] bf16 (nearest even)
__global__ void pack_weight_bf16_kernel(const float *__restrict__ w, int K, int CIN, int COUT, unsigned short *__restrict__ packed)
{
    const int total = K * CIN * COUT;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ci = i % CIN, co = (i / CIN) % COUT, k = i / (CIN * COUT);
    packed[i] = __builtin_bit_cast(unsigned short, (__bf16)w[((size_t)k * CIN + ci) * COUT + co]);
}

// densify of bf16 features: the bits copied into a bf16 map, or widened exactly into an fp32 map
template <typename TO>
__global__ void densify_from_bf16_kernel(const unsigned short *__restrict__ feats, const int32_t *__restrict__ idx,
                                         const int32_t *__restrict__ n_ptr, int cap, int C, int D, int H, int W, int order,
                                         TO *__restrict__ out)
{
    const int n = min(*n_ptr, cap);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * C) return;
    const int c = t / n, row = t - c * n;
    const int4 p = ((const int4 *)idx)[row];
    const int ch = order ? (p.y * C + c) : (c * D + p.y);
    const unsigned short v = feats[(size_t)row * C + c];
    if constexpr (sizeof(TO) == 2) out[(((size_t)p.x * C * D + ch) * H + p.z) * W + p.w] = v;
    else out[(((size_t)p.x * C * D + ch) * H + p.z) * W + p.w] = __uint_as_float((unsigned)v << 16);
}
