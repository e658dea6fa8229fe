// Metres -> the millimetres of the data set's depth PNGs (src/datasets/glassrgbd_norhint.py:273), shared by the dense
// post-processing (postproc.hip), the planar depth of the glass regions (regions.hip) and the fused sensor depth (fusion.hip) so that
// all of them agree bit for bit.
#pragma once
#include "common.h"

// rint(metres * 1000) as the PNGs hold it, saturated to the uint16 range
__device__ __forceinline__ unsigned short to_mm(float d) {
    const float mm = rintf(d * 1000.0f);
    return (unsigned short)fminf(fmaxf(mm, 0.0f), 65535.0f);
}
