// kitti_anno_core.h -- per-box arithmetic of the KITTI result annotation (include/sassd.h "KITTI annotations"): one
// lidar-frame detection -> camera-frame location / dimensions / rotation_y, alpha, and the 2-D box of its projected
// corners, with the keep test and the clip of kitti_common.kitti_bbox2results.  Written as __host__ __device__ functions
// so that the very same text is (a) called per thread by kitti_anno.hip and (b) looped over on the CPU by
// tests/kitti_anno_harness.hip, which checks it against kitti_bbox2results without a GPU.
//
// The dtype path is the host function's, step by step: the yaw wrap, the corners, sin / cos and alpha in float32; the
// lidar -> rect-camera transform and the projection in float64 (numpy promotes a float32 point joined to float64 ones).
// Products are rounded separately (no fused multiply-add) and every sum has one fixed association order, so the device
// and the CPU harness evaluate the same expression.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace sassd_kitti {

constexpr int kCalibDoubles = 36;       // Tr_velo_to_cam 12 | R0_rect 9 | P2 12 | img_w | img_h | pad

struct Anno {
    float cam[7];                       // x, y, z (rect camera), l, h, w, rotation_y
    float alpha;
    double bbox[4];                     // x1, y1, x2, y2, clipped to the image
    bool keep;                          // false: the projection misses the image (bbox is then unclipped)
};

// limit_period(yaw, 0.5, 2 pi) on a float32 array: the period is rounded to float32 first.
__host__ __device__ inline float wrap_yaw(float yaw)
{
#pragma clang fp contract(off)
    const float period = (float)(2.0 * 3.14159265358979323846);
    return yaw - floorf(yaw / period + 0.5f) * period;
}

// R0 . (V2C . [x y z 1]) in float64, rounded to float32 (the assignment into the float32 box array).
__host__ __device__ inline void lidar_to_rect(float x, float y, float z, const double *v2c, const double *r0, float *out)
{
#pragma clang fp contract(off)
    double c[3];
    for (int i = 0; i < 3; ++i)
        c[i] = (((double)x * v2c[4 * i] + (double)y * v2c[4 * i + 1]) + (double)z * v2c[4 * i + 2]) + v2c[4 * i + 3];
    for (int i = 0; i < 3; ++i) out[i] = (float)((c[0] * r0[3 * i] + c[1] * r0[3 * i + 1]) + c[2] * r0[3 * i + 2]);
}

// box = (x, y, z, w, l, h, yaw) in the lidar frame; calib = kCalibDoubles float64 as laid out above.
__host__ __device__ inline Anno box_anno(const float *box, const double *calib)
{
#pragma clang fp contract(off)
    const double *v2c = calib, *r0 = calib + 12, *p2 = calib + 21;
    const double img_w = calib[33], img_h = calib[34];
    Anno a;
    const float ry = wrap_yaw(box[6]);
    lidar_to_rect(box[0], box[1], box[2], v2c, r0, a.cam);
    a.cam[3] = box[4];
    a.cam[4] = box[5];
    a.cam[5] = box[3];
    a.cam[6] = ry;
    a.alpha = -atan2f(-box[1], box[0]) + ry;

    // _camera_box_corners: (unit offset - (0.5, 1, 0.5)) * (l, h, w), rotated about the camera y axis, + location
    const float s = sinf(ry), c = cosf(ry);
    double x1 = 0, y1 = 0, x2 = 0, y2 = 0;
    for (int k = 0; k < 8; ++k) {
        const float cx = a.cam[3] * ((k & 4) ? 0.5f : -0.5f);
        const float cy = a.cam[4] * ((k & 2) ? 0.f : -1.f);
        const float cz = a.cam[5] * ((k & 1) ? 0.5f : -0.5f);
        const float X = (cx * c + cz * s) + a.cam[0];
        const float Y = cy + a.cam[1];
        const float Z = (cx * (-s) + cz * c) + a.cam[2];
        // project_rect_to_image: P2 . [X Y Z 1] in float64, u and v divided by w
        const double u = (((double)X * p2[0] + (double)Y * p2[1]) + (double)Z * p2[2]) + p2[3];
        const double v = (((double)X * p2[4] + (double)Y * p2[5]) + (double)Z * p2[6]) + p2[7];
        const double w = (((double)X * p2[8] + (double)Y * p2[9]) + (double)Z * p2[10]) + p2[11];
        const double px = u / w, py = v / w;
        if (k == 0) {
            x1 = x2 = px;
            y1 = y2 = py;
        } else {
            if (px < x1) x1 = px;
            if (px > x2) x2 = px;
            if (py < y1) y1 = py;
            if (py > y2) y2 = py;
        }
    }
    a.keep = !(x1 > img_w || y1 > img_h || x2 < 0.0 || y2 < 0.0);
    a.bbox[0] = x1 < 0.0 ? 0.0 : x1;
    a.bbox[1] = y1 < 0.0 ? 0.0 : y1;
    a.bbox[2] = x2 > img_w ? img_w : x2;
    a.bbox[3] = y2 > img_h ? img_h : y2;
    return a;
}

}  // namespace sassd_kitti
