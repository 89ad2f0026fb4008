// TEST INFRASTRUCTURE (never linked into libsassd.so, never imported by the product path).
// Loops the product's __host__ __device__ test-time augmentation arithmetic on the CPU -- global_point of
// sa-ssd_amd/csrc/augment_core.h on the rows of a cloud, as one thread of tta_views_kernel applies it, and unview_box of
// sa-ssd_amd/csrc/tta_core.h on an array of boxes, as one thread of tta_pool_kernel applies it -- so that the arithmetic of the
// device path can be checked against sassd.tta.views_host / pool_host in the GPU-less test suite.  Built host-only
// (hipcc -x hip --cuda-host-only) by tests/tta_cases.py into a temporary directory.
#include "../sa-ssd_amd/csrc/augment_core.h"
#include "../sa-ssd_amd/csrc/tta_core.h"

extern "C" void hst_tta_view(const float *src, int n, int ndim, int flip, float s, float c, float scale, float *dst)
{
    for (int r = 0; r < n; ++r) {
        const uint32_t *in = reinterpret_cast<const uint32_t *>(src) + (size_t)r * ndim;
        uint32_t *out = reinterpret_cast<uint32_t *>(dst) + (size_t)r * ndim;
        float p[3] = {src[(size_t)r * ndim], src[(size_t)r * ndim + 1], src[(size_t)r * ndim + 2]};
        sassd_aug::global_point(p, flip, s, c, scale);
        for (int k = 0; k < 3; ++k) dst[(size_t)r * ndim + k] = p[k];
        for (int k = 3; k < ndim; ++k) out[k] = in[k];
    }
}

extern "C" void hst_tta_unview(float *boxes, int n, int flip, float s, float c, float scale, float angle)
{
    for (int i = 0; i < n; ++i) sassd_tta::unview_box(boxes + (size_t)i * 7, flip, s, c, scale, angle);
}
