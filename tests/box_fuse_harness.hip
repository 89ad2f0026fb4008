// TEST INFRASTRUCTURE (never linked into libsassd.so, never imported by the product path).
// Loops the product's __host__ __device__ box fusion rule on the CPU -- is_member, term, add, fusable and fused_field of
// sa-ssd_amd/csrc/box_fuse_core.h, as the lanes of box_fuse_kernel apply them to one detection: the members in ascending
// candidate row, sum q by "lane" q -- so that the arithmetic of the device path can be checked against
// sassd.fuse.fuse_host in the GPU-less test suite.  The scores and the IoU matrix are inputs, as they are of the rule.
// Built host-only (hipcc -x hip --cuda-host-only) by tests/box_fuse_cases.py into a temporary directory.
#include "../sa-ssd_amd/csrc/box_fuse_core.h"

#include <string.h>

extern "C" void hst_box_fuse(const float *guided, const float *scores, const int32_t *labels, int K, float score_thr,
                             float fuse_iou, const float *det_boxes, const int32_t *det_labels, int D, const float *iou,
                             float *fused)
{
    using namespace sassd_fuse;
    for (int t = 0; t < D; ++t) {
        const float *d = det_boxes + (size_t)t * 7;
        double sum[kSums] = {0, 0, 0, 0, 0, 0, 0, 0};
        int members = 0;
        for (int j = 0; j < K; ++j) {
            if (!is_member(scores[j], score_thr, labels[j], det_labels[t], iou[(size_t)t * K + j], fuse_iou)) continue;
            const float *f = guided + (size_t)j * 7;
            for (int q = 0; q < kSums; ++q) sum[q] = add(sum[q], members == 0, term(q, scores[j], q < 7 ? f[q] : 0.f, d[6]));
            ++members;
        }
        if (fusable(members, sum[kWeight])) {
            for (int q = 0; q < 7; ++q) fused[(size_t)t * 7 + q] = fused_field(q, sum[q], sum[kWeight], d[6]);
        } else {
            memcpy(fused + (size_t)t * 7, d, 7 * sizeof(float));
        }
    }
}
