// tta.hip -- test-time augmentation inside a captured frame (include/sassd.h "Test-time augmentation"): the two kernels
// between which the unchanged detector runs on V views of every cloud.
//
//   tta_views_kernel   behind the crop / merge nodes, in front of the voxelizer: the clouds of views 1 .. V-1 from the
//                      identity view's, global_point of augment_core.h on x, y, z, every further column copied.  Grid
//                      (ceil(cap * ndim / 256), V - 1); a thread owns ONE float of one destination, so that lane i of a
//                      wave reads and writes dword i of a contiguous run whatever the row width is (paste_objects_nd).
//   tta_pool_kernel    between PSWarp and rescore / NMS: the candidates of the V views of a sample, brought back into the
//                      sensor frame (unview_box of tta_core.h), as one view-major candidate list.  Grid
//                      (ceil(capP / 256), batch); a thread owns one pooled row and finds its view from the V <= 8 counts.
//
// Plain loads and vector stores; no workgroup waits for another, nothing is counted across workgroups, no memset, no
// atomics but the OR into the status word.
#include "augment_core.h"
#include "common.h"
#include "tta_core.h"

namespace {
using namespace sassd_tta;

constexpr int kThreads = 256;

struct ViewsArgs {
    const float *src;
    const int32_t *n_src;
    float *dst[kMaxViews - 1];
    int32_t *n_dst[kMaxViews - 1];
    int flip[kMaxViews - 1];
    float s[kMaxViews - 1], c[kMaxViews - 1], scale[kMaxViews - 1];
    int cap, ndim;
};

// W: the row width as a template argument (e / W is a multiply and a shift); 0: the runtime width a.ndim
template <int W>
__global__ void __launch_bounds__(kThreads) tta_views_kernel(ViewsArgs a)
{
    const int v = blockIdx.y;                                   // destination v is view v + 1; < V - 1 by the grid
    const int w = W ? W : a.ndim;
    int n = *a.n_src;
    n = n < 0 ? 0 : (n > a.cap ? a.cap : n);
    if (blockIdx.x == 0 && threadIdx.x == 0) *a.n_dst[v] = n;
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    const long long r = e / w;
    if (r >= n) return;
    const int col = (int)(e - r * w);
    const uint32_t *src = reinterpret_cast<const uint32_t *>(a.src) + r * w;
    uint32_t out = src[col];
    if (col < 3) {
        float p[3] = {__uint_as_float(src[0]), __uint_as_float(src[1]), __uint_as_float(src[2])};
        sassd_aug::global_point(p, a.flip[v], a.s[v], a.c[v], a.scale[v]);
        out = __float_as_uint(col == 0 ? p[0] : col == 1 ? p[1] : p[2]);
    }
    reinterpret_cast<uint32_t *>(a.dst[v])[e] = out;
}

struct PoolArgs {
    const float *guided, *logits;
    const int32_t *labels, *counts;
    float *guided_p, *logits_p;
    int32_t *labels_p, *counts_p, *status;
    int flip[kMaxViews];
    float s[kMaxViews], c[kMaxViews], scale[kMaxViews], angle[kMaxViews];
    int V, capK, capP;
};

__global__ void __launch_bounds__(kThreads) tta_pool_kernel(PoolArgs a)
{
    const int b = blockIdx.y;                                   // user sample; its views are inner samples b * V + v
    const int j = blockIdx.x * kThreads + threadIdx.x;          // pooled row
    int total = 0, view = -1, row = 0;
    for (int v = 0; v < a.V; ++v) {
        int c = a.counts[b * a.V + v];
        c = c < 0 ? 0 : (c > a.capK ? a.capK : c);
        if (view < 0 && j < total + c) { view = v; row = j - total; }
        total += c;
    }
    if (j == 0) {
        a.counts_p[b] = total < a.capP ? total : a.capP;
        if (total > a.capP) atomicOr(a.status, SASSD_ST_BOX_OVERFLOW);
    }
    if (view < 0 || j >= a.capP) return;
    const size_t src = (size_t)(b * a.V + view) * (size_t)a.capK + (size_t)row;
    const size_t dst = (size_t)b * (size_t)a.capP + (size_t)j;
    const uint32_t *g = reinterpret_cast<const uint32_t *>(a.guided) + src * 7;
    uint32_t *o = reinterpret_cast<uint32_t *>(a.guided_p) + dst * 7;
    if (view == 0) {                                            // the identity view: bit for bit
        for (int k = 0; k < 7; ++k) o[k] = g[k];
    } else {
        float box[7];
        for (int k = 0; k < 7; ++k) box[k] = __uint_as_float(g[k]);
        unview_box(box, a.flip[view], a.s[view], a.c[view], a.scale[view], a.angle[view]);
        for (int k = 0; k < 7; ++k) o[k] = __float_as_uint(box[k]);
    }
    reinterpret_cast<uint32_t *>(a.logits_p)[dst] = reinterpret_cast<const uint32_t *>(a.logits)[src];
    a.labels_p[dst] = a.labels[src];
}

// view 0 is the identity and every scale is a positive finite number
bool views_ok(int V, const int32_t *flip, const float *s, const float *c, const float *scale)
{
    if (flip[0] != 0 || s[0] != 0.f || c[0] != 1.f || scale[0] != 1.f) return false;
    for (int v = 0; v < V; ++v) {
        if (flip[v] != 0 && flip[v] != 1) return false;
        if (!(scale[v] > 0.f) || !(scale[v] <= 3.402823466e38f)) return false;
        if (!(s[v] >= -1.f && s[v] <= 1.f) || !(c[v] >= -1.f && c[v] <= 1.f)) return false;
    }
    return true;
}
}  // namespace

extern "C" int sassd_tta_views_dev(const float *src, int cap, const int32_t *n_src_dev, int ndim, int V,
                                   const int32_t *flip, const float *rot_sin, const float *rot_cos, const float *scale,
                                   float *const *dst, int32_t *const *n_dst_dev, int cap_dst, void *stream_)
{
    if (V < 1 || V > kMaxViews || ndim < 3 || cap < 1) return SASSD_EINVAL;
    if (!src || !n_src_dev || !flip || !rot_sin || !rot_cos || !scale) return SASSD_EINVAL;
    if (((uintptr_t)src | (uintptr_t)n_src_dev) & 3) return SASSD_EINVAL;
    if (!views_ok(V, flip, rot_sin, rot_cos, scale)) return SASSD_EINVAL;
    if (V == 1) return SASSD_OK;                                // the identity view is the source itself: nothing to write
    if (!dst || !n_dst_dev) return SASSD_EINVAL;
    ViewsArgs a;
    a.src = src; a.n_src = n_src_dev; a.cap = cap; a.ndim = ndim;
    for (int v = 0; v < kMaxViews - 1; ++v) {
        const bool used = v < V - 1;
        if (used && (!dst[v] || !n_dst_dev[v] || dst[v] == src || (((uintptr_t)dst[v] | (uintptr_t)n_dst_dev[v]) & 3)))
            return SASSD_EINVAL;
        a.dst[v] = used ? dst[v] : nullptr;
        a.n_dst[v] = used ? n_dst_dev[v] : nullptr;
        a.flip[v] = used ? flip[v + 1] : 0;
        a.s[v] = used ? rot_sin[v + 1] : 0.f;
        a.c[v] = used ? rot_cos[v + 1] : 1.f;
        a.scale[v] = used ? scale[v + 1] : 1.f;
    }
    if (cap_dst < cap) return SASSD_ENOSPC;
    const long long n_elem = (long long)cap * ndim;
    if (n_elem > (long long)0x7fffffff * kThreads) return SASSD_EINVAL;         // the grid's x extent
    const dim3 grid((unsigned)((n_elem + kThreads - 1) / kThreads), V - 1), block(kThreads);   // a function of (cap, ndim, V)
    hipStream_t s = (hipStream_t)stream_;
    switch (ndim) {
    case 3: hipLaunchKernelGGL(tta_views_kernel<3>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(tta_views_kernel<4>, grid, block, 0, s, a); break;
    case 5: hipLaunchKernelGGL(tta_views_kernel<5>, grid, block, 0, s, a); break;
    case 6: hipLaunchKernelGGL(tta_views_kernel<6>, grid, block, 0, s, a); break;
    case 7: hipLaunchKernelGGL(tta_views_kernel<7>, grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL(tta_views_kernel<8>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(tta_views_kernel<0>, grid, block, 0, s, a); break;
    }
    return sassd_launch_status();
}

extern "C" int sassd_tta_pool(const float *guided, const float *logits, const int32_t *labels, const int32_t *counts,
                              int batch, int V, int capK, const int32_t *flip, const float *rot_sin, const float *rot_cos,
                              const float *scale, const float *angle, float *guided_p, float *logits_p, int32_t *labels_p,
                              int32_t *counts_p, int capP, int32_t *status, void *stream_)
{
    if (V < 1 || V > kMaxViews || batch < 1 || capK < 1 || capP < 1 || capP > 4096) return SASSD_EINVAL;
    if (!guided || !logits || !labels || !counts || !flip || !rot_sin || !rot_cos || !scale || !angle || !guided_p ||
        !logits_p || !labels_p || !counts_p || !status)
        return SASSD_EINVAL;
    if (((uintptr_t)guided | (uintptr_t)logits | (uintptr_t)labels | (uintptr_t)counts | (uintptr_t)guided_p |
         (uintptr_t)logits_p | (uintptr_t)labels_p | (uintptr_t)counts_p | (uintptr_t)status) & 3)
        return SASSD_EINVAL;
    if ((long long)batch * V > 0x7fffffff / 4096) return SASSD_EINVAL;
    if (!views_ok(V, flip, rot_sin, rot_cos, scale)) return SASSD_EINVAL;
    for (int v = 0; v < V; ++v)
        if (!(angle[v] >= -3.402823466e38f && angle[v] <= 3.402823466e38f)) return SASSD_EINVAL;
    if (angle[0] != 0.f) return SASSD_EINVAL;
    if (capP < (capK < 4096 ? capK : 4096)) return SASSD_ENOSPC;       // the pool holds at least the identity view, whole
    PoolArgs a;
    a.guided = guided; a.logits = logits; a.labels = labels; a.counts = counts;
    a.guided_p = guided_p; a.logits_p = logits_p; a.labels_p = labels_p; a.counts_p = counts_p; a.status = status;
    a.V = V; a.capK = capK; a.capP = capP;
    for (int v = 0; v < kMaxViews; ++v) {
        const bool used = v < V;
        a.flip[v] = used ? flip[v] : 0;
        a.s[v] = used ? rot_sin[v] : 0.f;
        a.c[v] = used ? rot_cos[v] : 1.f;
        a.scale[v] = used ? scale[v] : 1.f;
        a.angle[v] = used ? angle[v] : 0.f;
    }
    hipLaunchKernelGGL(tta_pool_kernel, dim3(cdiv(capP, kThreads), batch), dim3(kThreads), 0, (hipStream_t)stream_, a);
    return sassd_launch_status();
}
