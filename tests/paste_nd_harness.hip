// TEST INFRASTRUCTURE: the product's __host__ __device__ paste arithmetic (sa-ssd_amd/csrc/augment_core.h: object_of_row,
// paste_point_nd) looped on the CPU over one case of tests/wide_cloud_cases.py -- the loop of paste_objects_nd_kernel with
// a row per iteration.  Built with `hipcc --cuda-host-only` by wide_cloud_cases.harness; needs no GPU.
#include "../sa-ssd_amd/csrc/augment_core.h"

using namespace sassd_aug;

extern "C" void hst_paste_objects_nd(const float *db_points, int ndim, const int64_t *src_start, const int64_t *out_start,
                                     int n_obj, int64_t n_out, const double *shift, const double *lower, float *out)
{
    for (int64_t r = 0; r < n_out; ++r) {
        const int k = object_of_row(out_start, n_obj, r);
        paste_point_nd(db_points + (src_start[k] + (r - out_start[k])) * ndim, out + r * ndim, ndim, shift + 3 * k,
                       lower ? lower + k : nullptr);
    }
}
