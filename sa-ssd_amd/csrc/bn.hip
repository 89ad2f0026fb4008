// bn.hip -- training-mode BatchNorm1d + ReLU over sparse-tensor features [N, C] (row-major), forward and backward.
//
// The reference's sparse blocks are  SubMConv3d / SparseConv3d -> BatchNorm1d(eps 1e-3, momentum 0.01) -> ReLU
// (mmdet/models/necks/cmn.py:147-173 through spconv.SparseSequential): in training mode torch runs them as
// collect-statistics + transform + clamp (forward) and threshold + reduce + elementwise (backward), six launches per
// layer over a 1-9 MB tensor, i.e. launch latency.  Here: three short launches each way.
//   forward   bn_stats_kernel      per-channel sum / sum of squares (16-byte loads, <= 16 elements in fp32, then double)
//                                  -> one partial pair per block and channel
//             bn_finalize_kernel   one block PER CHANNEL adds the <= 1024 block partials in a fixed order (deterministic):
//                                  mean / invstd, running statistics (unbiased variance, like torch).  (Round 2 let every
//                                  block of the apply launch redo this reduction -- 256 KB of partials per block: 18 us
//                                  per launch instead of 6; rounds 2-4 used ONE block for all channels: 8.8 us of
//                                  dependent-load latency.)
//             bn_apply_relu_kernel y = max(0, (x - mean) * (invstd * gamma) + beta)
//   backward  bn_bwd_reduce_kernel dz = dy * (z > 0) with z recomputed from x exactly as the forward computed it;
//                                  partials of sum dz, sum dz * xhat
//             bn_bwd_finalize_kernel  -> dbeta, dgamma
//             bn_bwd_apply_kernel  dx = gamma * invstd * (dz - dbeta / N - xhat * dgamma / N)
// C is a multiple of 4 and at most 256 (the sparse trunk has 16 / 32 / 64).
#include "common.h"

namespace {
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kBnMaxBlocks = 1024;     // (317 k-row Waymo-scale levels: 256 blocks walked 1240 rows each)

struct BnFwdArgs {
    const float *x;
    int n, C, nb, rows_per_block;
    double *part;            // [nb][2][C]
    float *mean, *invstd;    // [C] saved for the backward pass
    float *rmean, *rvar;     // running statistics (may be null)
    float momentum, eps;
};

// block-wide sum of two doubles (256 threads, fixed xor-shuffle tree + the four wave results in wave order); valid in thread 0
__device__ __forceinline__ void bn_block_sum2(double &a, double &b, double (*red)[4])
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][w] = a; red[1][w] = b; }
    __syncthreads();
    a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    b = red[1][0] + red[1][1] + red[1][2] + red[1][3];
}

// 256 threads = (1024 / C) row lanes x C / 4 channel quads: one 16-byte load per thread and row (round 5; rounds 2-4 loaded
// 4 bytes per thread and converted every element to double: 7.1 us at 36 k x 64).  A thread adds <= 16 elements per channel
// in fp32 before it widens (like bn2d_stats_kernel); the row lanes of a channel are added in lane order.
__global__ void __launch_bounds__(256) bn_stats_kernel(BnFwdArgs P)
{
    __shared__ double red[4][4][256];
    const int C = P.C, C4 = C >> 2, rl = 256 / C4;
    const int c4 = threadIdx.x % C4, r = threadIdx.x / C4;
    const int r0 = blockIdx.x * P.rows_per_block, r1 = min(r0 + P.rows_per_block, P.n);
    double ds[4] = {0.0, 0.0, 0.0, 0.0}, dq[4] = {0.0, 0.0, 0.0, 0.0};
    f32x4 fs = {0.f, 0.f, 0.f, 0.f}, fq = fs;
    int cnt = 0;
    // Round 6: next to the raw sums a thread keeps fp32 sums of the RESIDUALS to the first value it loads and
    // re-bases them to zero in double (sum x^2 = sum d^2 + 2 s sum d + k s^2, d = x - s): their fp32 rounding acts on the local
    // variation of the channel, not on its mean^2.  bn_finalize_kernel takes the variance from them ONLY where the raw form
    // cancels (mean^2 > 1024 var: a channel with mean 40 and variance 1e-2 lost ~1 % of its invstd) -- everywhere else the
    // statistics keep the bits of rounds 2-5.  (Two simpler versions were measured first: one shift per channel = its first row is
    // WORSE than no shift when that row is an outlier; residual sums everywhere are 1e-7 from float64 like the raw ones
    // (tests/analysis/bn_stats_probe.py), but any change of their last bits moves the synthetic full-grid multi_cfg training step
    // across some discontinuity of its backward pass -- losses equal to 1e-7, whole-model gradient 1.5e-4 -> 7.7e-4 from the float64
    // arbiter, uniformly below the rescoring head -- so the bits of the normal regime stay what every arbiter test was run on.)
    double d1[4] = {0.0, 0.0, 0.0, 0.0}, d2[4] = {0.0, 0.0, 0.0, 0.0};     // re-based sum x / sum x^2 (both: the mean of the
    f32x4 sh = {0.f, 0.f, 0.f, 0.f}, rs = sh, rq = sh;                      // cancelling regime must be as exact as its squares)
    bool have = false;
    for (int row = r0 + r; row < r1; row += rl) {
        const f32x4 v = ((const f32x4 *)P.x)[(size_t)row * C4 + c4];
        if (!have) { sh = v; have = true; }
        const f32x4 d = v - sh;
        fs += v;
        fq += v * v;
        rs += d;
        rq += d * d;
        if (++cnt == 16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                ds[j] += (double)fs[j]; dq[j] += (double)fq[j];
                d1[j] += (double)rs[j] + 16.0 * (double)sh[j];
                d2[j] += (double)rq[j] + 2.0 * (double)sh[j] * (double)rs[j] + 16.0 * (double)sh[j] * (double)sh[j];
            }
            fs = fq = rs = rq = (f32x4){0.f, 0.f, 0.f, 0.f};
            cnt = 0;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[0][j][threadIdx.x] = ds[j] + (double)fs[j];
        red[1][j][threadIdx.x] = dq[j] + (double)fq[j];
        red[2][j][threadIdx.x] = d2[j] + (double)rq[j] + 2.0 * (double)sh[j] * (double)rs[j] + cnt * (double)sh[j] * (double)sh[j];
        red[3][j][threadIdx.x] = d1[j] + (double)rs[j] + cnt * (double)sh[j];
    }
    __syncthreads();
    if (threadIdx.x < C) {
        const int q = threadIdx.x >> 2, j = threadIdx.x & 3;
        double ss = 0.0, qq = 0.0, q2 = 0.0, s2 = 0.0;
        for (int k = 0; k < rl; ++k) {
            ss += red[0][j][k * C4 + q]; qq += red[1][j][k * C4 + q]; q2 += red[2][j][k * C4 + q]; s2 += red[3][j][k * C4 + q];
        }
        P.part[((size_t)blockIdx.x * 2 + 0) * C + threadIdx.x] = ss;
        P.part[((size_t)blockIdx.x * 2 + 1) * C + threadIdx.x] = qq;
        // the re-based pair: a second [nb][2][C] block behind the first
        P.part[(size_t)kBnMaxBlocks * 2 * C + ((size_t)blockIdx.x * 2 + 0) * C + threadIdx.x] = s2;
        P.part[(size_t)kBnMaxBlocks * 2 * C + ((size_t)blockIdx.x * 2 + 1) * C + threadIdx.x] = q2;
    }
}

// sums of the block partials of ONE channel (block c of the finalize launches; 256 threads): thread t adds the partials of
// blocks t, t + 256, ... in order, then the fixed block tree.  (Rounds 2-4: one 1024-thread block for all channels walked
// <= 1024 / (1024 / C) dependent loads per thread -- 8.8 us of load latency per call; C blocks: one to four loads.)
__device__ __forceinline__ void bn_reduce_channel(const double *part, int nb, int C, int c, double (*red)[4], double &a, double &b)
{
    a = 0.0; b = 0.0;
    for (int k = threadIdx.x; k < nb; k += 256) {
        a += part[((size_t)k * 2 + 0) * C + c];
        b += part[((size_t)k * 2 + 1) * C + c];
    }
    bn_block_sum2(a, b, red);
}

struct BnApplyArgs {
    const float *x;
    int n, C, nb;
    const double *part;
    const float *gamma, *beta;
    void *y;                 // fp32, or bf16 (nearest even) for the _bf16out entry points
    float *mean, *invstd, *rmean, *rvar;
    float momentum, eps;
};

// the one store of the two apply kernels: four channels of a row as fp32, or rounded to bf16 (nearest even) by a plain cast
template <typename TO>
__device__ __forceinline__ void bn_store4(void *dst, size_t i, const f32x4 &o)
{
    if constexpr (sizeof(TO) == 4) {
        ((f32x4 *)dst)[i] = o;
    } else {
        ((ushort4 *)dst)[i] = make_ushort4(__builtin_bit_cast(unsigned short, (__bf16)o[0]), __builtin_bit_cast(unsigned short, (__bf16)o[1]),
                                           __builtin_bit_cast(unsigned short, (__bf16)o[2]), __builtin_bit_cast(unsigned short, (__bf16)o[3]));
    }
}

__global__ void __launch_bounds__(256) bn_finalize_kernel(BnApplyArgs P)
{
    __shared__ double red[2][4];
    const int c = blockIdx.x;
    double ss, qq;
    bn_reduce_channel(P.part, P.nb, P.C, c, red, ss, qq);
    __syncthreads();
    double s2, q2;                                       // the re-based pair, same fixed order
    bn_reduce_channel(P.part + (size_t)kBnMaxBlocks * 2 * P.C, P.nb, P.C, c, red, s2, q2);
    if (threadIdx.x == 0) {
        double mean = ss / P.n;
        double var = qq / P.n - mean * mean;
        // the raw form cancels: see bn_stats_kernel.  Up to 1024 / C rows (one block, at most one row per thread) the re-based
        // pair is EXACT -- a thread's residuals are zero and its shift is squared in double -- while the raw one carries the fp32
        // rounding of every x^2 with no other row to average it out: two rows with mean^2 = 500 var lost 2e-5 of their variance
        // (tests/test_gpu_backbone_grad_kernels.py, n = 2 .. 4).  No layer of a real frame is that short: their bits stay.
        if (mean * mean > 1024.0 * var || P.n <= 1024 / P.C) {
            mean = s2 / P.n;
            var = q2 / P.n - mean * mean;
        }
        if (var < 0.0) var = 0.0;
        P.mean[c] = (float)mean;
        P.invstd[c] = (float)(1.0 / sqrt(var + (double)P.eps));
        if (P.rmean) {
            const double unb = P.n > 1 ? var * P.n / (P.n - 1) : var;
            P.rmean[c] = (float)((1.0 - P.momentum) * P.rmean[c] + P.momentum * mean);
            P.rvar[c] = (float)((1.0 - P.momentum) * P.rvar[c] + P.momentum * unb);
        }
    }
}

template <typename TO>
__global__ void __launch_bounds__(256) bn_apply_relu_kernel(BnApplyArgs P)
{
    __shared__ float s_mean[256], s_scale[256], s_shift[256];
    const int C = P.C;
    if (threadIdx.x < C) {
        s_mean[threadIdx.x] = P.mean[threadIdx.x];
        s_scale[threadIdx.x] = P.invstd[threadIdx.x] * P.gamma[threadIdx.x];
        s_shift[threadIdx.x] = P.beta[threadIdx.x];
    }
    __syncthreads();
    const size_t total = (size_t)P.n * C / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)((i * 4) % C);
        const f32x4 v = ((const f32x4 *)P.x)[i];             // one float4 = 4 channels of one row
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float z = fmaf(v[j] - s_mean[c + j], s_scale[c + j], s_shift[c + j]);   // (= the backward's expression)
            o[j] = z > 0.f ? z : 0.f;
        }
        bn_store4<TO>(P.y, i, o);
    }
}

struct BnBwdArgs {
    const float *x, *dy;
    int n, C, nb, rows_per_block;
    const float *mean, *invstd, *gamma, *beta;
    double *part;            // [nb][2][C]
    void *dx;                // fp32, or bf16 (nearest even) for the _bf16out entry points
    float *dgamma, *dbeta;
};

__global__ void __launch_bounds__(256) bn_bwd_reduce_kernel(BnBwdArgs P)
{
    __shared__ double red[2][4][256];
    const int C = P.C, C4 = C >> 2, rl = 256 / C4;
    const int c4 = threadIdx.x % C4, r = threadIdx.x / C4;
    const int r0 = blockIdx.x * P.rows_per_block, r1 = min(r0 + P.rows_per_block, P.n);
    float m[4], is[4], g[4], bt[4];                 // (scalar loads: gamma / beta are views into the flat parameter buffer,
#pragma unroll                                      //  at any 4-byte offset)
    for (int j = 0; j < 4; ++j) {
        m[j] = P.mean[c4 * 4 + j]; is[j] = P.invstd[c4 * 4 + j]; g[j] = P.gamma[c4 * 4 + j]; bt[j] = P.beta[c4 * 4 + j];
    }
    double db[4] = {0.0, 0.0, 0.0, 0.0}, dg[4] = {0.0, 0.0, 0.0, 0.0};
    f32x4 fb = {0.f, 0.f, 0.f, 0.f}, fg = fb;
    int cnt = 0;
    for (int row = r0 + r; row < r1; row += rl) {
        const f32x4 xv = ((const f32x4 *)P.x)[(size_t)row * C4 + c4], d = ((const f32x4 *)P.dy)[(size_t)row * C4 + c4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (xv[j] - m[j]) * is[j];
            const float z = fmaf(xv[j] - m[j], is[j] * g[j], bt[j]);     // exactly the forward's z: the mask is y > 0
            const float dz = z > 0.f ? d[j] : 0.f;
            fb[j] += dz;
            fg[j] += dz * xh;
        }
        if (++cnt == 16) {
#pragma unroll
            for (int j = 0; j < 4; ++j) { db[j] += (double)fb[j]; dg[j] += (double)fg[j]; }
            fb = fg = (f32x4){0.f, 0.f, 0.f, 0.f};
            cnt = 0;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        red[0][j][threadIdx.x] = db[j] + (double)fb[j];
        red[1][j][threadIdx.x] = dg[j] + (double)fg[j];
    }
    __syncthreads();
    if (threadIdx.x < C) {
        const int q = threadIdx.x >> 2, j = threadIdx.x & 3;
        double a = 0.0, b = 0.0;
        for (int k = 0; k < rl; ++k) { a += red[0][j][k * C4 + q]; b += red[1][j][k * C4 + q]; }
        P.part[((size_t)blockIdx.x * 2 + 0) * C + threadIdx.x] = a;
        P.part[((size_t)blockIdx.x * 2 + 1) * C + threadIdx.x] = b;
    }
}

__global__ void __launch_bounds__(256) bn_bwd_finalize_kernel(BnBwdArgs P)
{
    __shared__ double red[2][4];
    double a, b;
    bn_reduce_channel(P.part, P.nb, P.C, blockIdx.x, red, a, b);
    if (threadIdx.x == 0) {
        P.dbeta[blockIdx.x] = (float)a;
        P.dgamma[blockIdx.x] = (float)b;
    }
}

template <typename TO>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(BnBwdArgs P)
{
    __shared__ float s_mean[256], s_is[256], s_g[256], s_b[256], s_db[256], s_dg[256];
    const int C = P.C;
    if (threadIdx.x < C) {
        s_mean[threadIdx.x] = P.mean[threadIdx.x];
        s_is[threadIdx.x] = P.invstd[threadIdx.x];
        s_g[threadIdx.x] = P.gamma[threadIdx.x];
        s_b[threadIdx.x] = P.beta[threadIdx.x];
        s_db[threadIdx.x] = P.dbeta[threadIdx.x];
        s_dg[threadIdx.x] = P.dgamma[threadIdx.x];
    }
    __syncthreads();
    const float inv_n = 1.f / (float)P.n;
    const size_t total = (size_t)P.n * C / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const int c = (int)((i * 4) % C);
        const f32x4 v = ((const f32x4 *)P.x)[i], g = ((const f32x4 *)P.dy)[i];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (v[j] - s_mean[c + j]) * s_is[c + j];
            const float z = fmaf(v[j] - s_mean[c + j], s_is[c + j] * s_g[c + j], s_b[c + j]);
            const float dz = z > 0.f ? g[j] : 0.f;
            o[j] = s_g[c + j] * s_is[c + j] * (dz - s_db[c + j] * inv_n - xh * s_dg[c + j] * inv_n);
        }
        bn_store4<TO>(P.dx, i, o);
    }
}

int bn_blocks(int n, int C, int *rows_per_block)
{
    const int rl = 1024 / C;                         // rows one block covers per iteration (a 16-byte load per thread)
    int it = n / (512 * rl);                         // ~512 blocks (two per CU) ...
    it = it < 2 ? 2 : (it > 16 ? 16 : it);           // ... of 2 .. 16 row iterations
    int nb = cdiv(n, it * rl);
    nb = nb < 1 ? 1 : (nb > kBnMaxBlocks ? kBnMaxBlocks : nb);
    *rows_per_block = cdiv(n, nb);
    return cdiv(n, *rows_per_block);
}
int bn_apply_blocks(int n, int C)
{
    const size_t total = (size_t)n * C / 4;
    const size_t nb = (total + 511) / 512;           // 2 float4 per thread
    return (int)(nb < 1 ? 1 : (nb > 2048 ? 2048 : nb));
}
bool bn_shape_ok(int n, int C) { return n >= 1 && C >= 4 && C <= 256 && C % 4 == 0 && 256 % C == 0; }
}  // namespace

extern "C" size_t sassd_bn_relu_workspace_bytes(int C)
{
    return C < 1 ? 0 : align_up((size_t)kBnMaxBlocks * 4 * C * sizeof(double), 256);
}

static int bn_relu_fwd_any(const float *x, int n, int C, const float *gamma, const float *beta,
                                 float *running_mean, float *running_var, float momentum, float eps, void *y, int y_bf16,
                                 float *save_mean, float *save_invstd, void *workspace, size_t workspace_bytes,
                                 void *stream_)
{
    if (y_bf16 && ((uintptr_t)y & 7)) return SASSD_EINVAL;
    if (!x || !gamma || !beta || !y || !save_mean || !save_invstd || !workspace || !bn_shape_ok(n, C) ||
        (!running_mean) != (!running_var))
        return SASSD_EINVAL;
    if (workspace_bytes < sassd_bn_relu_workspace_bytes(C)) return SASSD_ENOSPC;
    hipStream_t s = (hipStream_t)stream_;
    BnFwdArgs P;
    P.x = x; P.n = n; P.C = C;
    P.nb = bn_blocks(n, C, &P.rows_per_block);
    P.part = (double *)workspace;
    P.mean = save_mean; P.invstd = save_invstd; P.rmean = running_mean; P.rvar = running_var;
    P.momentum = momentum; P.eps = eps;
    hipLaunchKernelGGL(bn_stats_kernel, dim3(P.nb), dim3(256), 0, s, P);
    BnApplyArgs Q;
    Q.x = x; Q.n = n; Q.C = C; Q.nb = P.nb; Q.part = (const double *)workspace; Q.gamma = gamma; Q.beta = beta; Q.y = y;
    Q.mean = save_mean; Q.invstd = save_invstd; Q.rmean = running_mean; Q.rvar = running_var;
    Q.momentum = momentum; Q.eps = eps;
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(C), dim3(256), 0, s, Q);
    if (y_bf16) hipLaunchKernelGGL(bn_apply_relu_kernel<unsigned short>, dim3(bn_apply_blocks(n, C)), dim3(256), 0, s, Q);
    else hipLaunchKernelGGL(bn_apply_relu_kernel<float>, dim3(bn_apply_blocks(n, C)), dim3(256), 0, s, Q);
    return sassd_launch_status();
}

extern "C" int sassd_bn_relu_fwd(const float *x, int n, int C, const float *gamma, const float *beta,
                                 float *running_mean, float *running_var, float momentum, float eps, float *y,
                                 float *save_mean, float *save_invstd, void *workspace, size_t workspace_bytes,
                                 void *stream_)
{
    return bn_relu_fwd_any(x, n, C, gamma, beta, running_mean, running_var, momentum, eps, y, 0, save_mean, save_invstd, workspace,
                           workspace_bytes, stream_);
}

// sassd_bn_relu_fwd with the output rounded to bf16 (nearest even) at the store: the same statistics, the same arithmetic
extern "C" int sassd_bn_relu_fwd_bf16out(const float *x, int n, int C, const float *gamma, const float *beta,
                                         float *running_mean, float *running_var, float momentum, float eps, void *y_bf16,
                                         float *save_mean, float *save_invstd, void *workspace, size_t workspace_bytes,
                                         void *stream_)
{
    if ((uintptr_t)x & 15) return SASSD_EINVAL;
    return bn_relu_fwd_any(x, n, C, gamma, beta, running_mean, running_var, momentum, eps, y_bf16, 1, save_mean, save_invstd,
                           workspace, workspace_bytes, stream_);
}

static int bn_relu_bwd_any(const float *x, const float *dy, int n, int C, const float *gamma, const float *beta,
                                 const float *save_mean, const float *save_invstd, void *dx, int dx_bf16, float *dgamma,
                                 float *dbeta, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (dx_bf16 && ((uintptr_t)dx & 7)) return SASSD_EINVAL;
    if (!x || !dy || !gamma || !beta || !save_mean || !save_invstd || !dx || !dgamma || !dbeta || !workspace ||
        !bn_shape_ok(n, C))
        return SASSD_EINVAL;
    if (workspace_bytes < sassd_bn_relu_workspace_bytes(C)) return SASSD_ENOSPC;
    hipStream_t s = (hipStream_t)stream_;
    BnBwdArgs P;
    P.x = x; P.dy = dy; P.n = n; P.C = C;
    P.nb = bn_blocks(n, C, &P.rows_per_block);
    P.mean = save_mean; P.invstd = save_invstd; P.gamma = gamma; P.beta = beta;
    P.part = (double *)workspace;
    P.dx = dx; P.dgamma = dgamma; P.dbeta = dbeta;
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(P.nb), dim3(256), 0, s, P);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(C), dim3(256), 0, s, P);
    if (dx_bf16) hipLaunchKernelGGL(bn_bwd_apply_kernel<unsigned short>, dim3(bn_apply_blocks(n, C)), dim3(256), 0, s, P);
    else hipLaunchKernelGGL(bn_bwd_apply_kernel<float>, dim3(bn_apply_blocks(n, C)), dim3(256), 0, s, P);
    return sassd_launch_status();
}

extern "C" int sassd_bn_relu_bwd(const float *x, const float *dy, int n, int C, const float *gamma, const float *beta,
                                 const float *save_mean, const float *save_invstd, float *dx, float *dgamma,
                                 float *dbeta, void *workspace, size_t workspace_bytes, void *stream_)
{
    return bn_relu_bwd_any(x, dy, n, C, gamma, beta, save_mean, save_invstd, dx, 0, dgamma, dbeta, workspace, workspace_bytes,
                           stream_);
}

// sassd_bn_relu_bwd with dx rounded to bf16 (nearest even) at the store; dgamma / dbeta are its fp32 values bit for bit
extern "C" int sassd_bn_relu_bwd_bf16out(const float *x, const float *dy, int n, int C, const float *gamma, const float *beta,
                                         const float *save_mean, const float *save_invstd, void *dx_bf16, float *dgamma,
                                         float *dbeta, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (((uintptr_t)x | (uintptr_t)dy) & 15) return SASSD_EINVAL;
    return bn_relu_bwd_any(x, dy, n, C, gamma, beta, save_mean, save_invstd, dx_bf16, 1, dgamma, dbeta, workspace, workspace_bytes,
                           stream_);
}
