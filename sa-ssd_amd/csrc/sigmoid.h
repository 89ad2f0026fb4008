// sigmoid.h -- the fp32 sigmoid that turns a classification or rescoring logit into a score, stated once: decode + filter and
// rescore + NMS (heads.hip) and the box fusion behind them (box_fuse.hip) must give one logit one score.
#pragma once
#include <hip/hip_runtime.h>

namespace {
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }
}  // namespace
