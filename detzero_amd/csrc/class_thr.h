// Per-class thresholds passed to a kernel by value (track.hip, traj_pair.hip).
#pragma once
#include "common.h"

namespace dz {

struct ClassThr { float v[DZ_TRACK_MAX_CLASSES]; };

// thr.v[c] by a select chain: a dynamically indexed by-value struct would go through scratch memory (box_geom.h, rect_overlap)
__device__ __forceinline__ float thr_of(const ClassThr &thr, int c) {
    float t = thr.v[0];
#pragma unroll
    for (int k = 1; k < DZ_TRACK_MAX_CLASSES; ++k) t = c == k ? thr.v[k] : t;
    return t;
}

}  // namespace dz
