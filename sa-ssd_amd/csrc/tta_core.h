// tta_core.h -- per-box arithmetic of test-time augmentation (include/sassd.h "Test-time augmentation"): a candidate box
// found in a transformed copy of the cloud is brought back into the sensor frame.  The forward direction, on points, is
// global_point of augment_core.h.  Written as __host__ __device__ functions so that the very same text is (a) called per
// thread by tta.hip and (b) looped over on the CPU by tests/tta_harness.hip, which checks it against the numpy statement
// sassd.tta.pool_host without a GPU.
//
// A view is (flip, angle, scale); the host hands it over as flip, s = float32(sin(angle)), c = float32(cos(angle)),
// scale = float32(scale) and angle = float32(angle).  Everything is float32, every product, quotient and sum is rounded on
// its own (no fused multiply-add) and in one fixed order, so the device and the CPU harness evaluate the same expression.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sassd_tta {

constexpr int kMaxViews = 8;

// The inverses of random_flip, global_rotation and global_scaling as point_augmentor.py applies them to gt_boxes, in the
// reverse order: box = (x, y, z, w, l, h, yaw) of the view's frame -> the same box in the sensor frame, in place.
__host__ __device__ inline void unview_box(float *box, int flip, float s, float c, float scale, float angle)
{
#pragma clang fp contract(off)
    for (int k = 0; k < 6; ++k) box[k] = box[k] / scale;            // global_scaling: gt_boxes[:, :6] *= scale
    const float x = box[0], y = box[1];
    box[0] = x * c - y * s;                                         // global_rotation: [x y] @ [[c, -s], [s, c]] undone
    box[1] = x * s + y * c;
    box[6] = box[6] - angle;                                        //                  gt_boxes[:, 6] += angle
    if (flip) {
        box[1] = -box[1];                                           // random_flip: y = -y, yaw = -yaw + pi
        box[6] = -box[6] + 3.14159265358979323846f;
    }
}

}  // namespace sassd_tta
