// The points-in-boxes inside test (roiaware_pool3d_kernel.cu:26-45 check_pt_in_box3d as points_in_boxes_gpu_v2 uses it), one body for
// every kernel that decides membership: k_points_in_boxes / _bits / _count (head_post.hip) and the sequence crop (seq_crop.hip).
// A box is staged as 9 floats: its 7 parameters, then cosf(-yaw), sinf(-yaw).
#pragma once
#include <hip/hip_runtime.h>

namespace dz {

constexpr int PIB_BOX_FLOATS = 9;
constexpr int PIB_STAGE_BOXES = 64;           // boxes staged in LDS per round

__device__ __forceinline__ void pib_stage_box(const float *__restrict__ q, float *__restrict__ d) {
    for (int j = 0; j < 7; ++j) d[j] = q[j];
    d[7] = cosf(-q[6]);
    d[8] = sinf(-q[6]);
}

// z half-height compared in double; x / y in the box frame against half sizes + 1e-5f, in double
__device__ __forceinline__ bool pib_inside(float x, float y, float z, const float *__restrict__ q) {
#pragma clang fp contract(off)                // the reference's two roundings per product-sum, whatever the including file sets
    bool in = false;
    if (!((double)fabsf(z - q[2]) > (double)q[5] / 2.0)) {
        const float sx = x - q[0], sy = y - q[1];
        const float lx = sx * q[7] + sy * (-q[8]);
        const float ly = sx * q[8] + sy * q[7];
        in = ((double)fabsf(lx) < (double)q[3] / 2.0 + (double)1e-5f) && ((double)fabsf(ly) < (double)q[4] / 2.0 + (double)1e-5f);
    }
    return in;
}

}  // namespace dz
