// TEST INFRASTRUCTURE (never linked into libsassd.so, never imported by the product path).
// Loops box_anno of sa-ssd_amd/csrc/kitti_anno_core.h -- the exact code the kernel of kitti_anno.hip calls per thread --
// over an array of boxes on the CPU, so that the arithmetic of the device path can be checked against
// kitti_common.kitti_bbox2results in the GPU-less test suite.  Built host-only (hipcc -x hip --cuda-host-only) by
// tests/kitti_anno_cases.py into a temporary directory.
#include "../sa-ssd_amd/csrc/kitti_anno_core.h"

using namespace sassd_kitti;

extern "C" void hst_box_annos(const float *boxes, int n, const double *calib, float *cam, float *alpha, double *bbox,
                              uint8_t *keep)
{
    for (int i = 0; i < n; ++i) {
        const Anno a = box_anno(boxes + (size_t)i * 7, calib);
        for (int k = 0; k < 7; ++k) cam[(size_t)i * 7 + k] = a.cam[k];
        alpha[i] = a.alpha;
        for (int k = 0; k < 4; ++k) bbox[(size_t)i * 4 + k] = a.bbox[k];
        keep[i] = a.keep ? 1 : 0;
    }
}
