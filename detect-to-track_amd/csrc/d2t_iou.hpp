// d2t_iou.hpp -- the one IoU decision of the library: the region filter's NMS (d2t_regions.hip) and the tubelet
// linker's track matches (d2t_link.hip) both call iou_exceeds, so the two make the same decision for the same boxes.
// Boxes are (centre_i, centre_j, height, width); the expression is oracle/regions.py:iou_one_to_many's, float32 throughout,
// and symmetric in its two boxes (fminf / fmaxf and the sum of the two areas commute).
#pragma once
#include <hip/hip_runtime.h>

namespace d2t {

// IoU(a, b) > thr, decided as the float quotient inter / uni would decide it (oracle/regions.py: float32 throughout).
// The quotient is first estimated with v_rcp_f32 (error of a few 1e-7 for a value in [0, 1]); the IEEE division runs
// only when the estimate is within 1e-6 of the threshold or not a number (uni <= 0: the pair scores 0).
__device__ __forceinline__ bool iou_exceeds(const float4& a, const float4& b, float thr)
{
    const float ai0 = a.x - a.z / 2.f, ai1 = a.x + a.z / 2.f, aj0 = a.y - a.w / 2.f, aj1 = a.y + a.w / 2.f;
    const float bi0 = b.x - b.z / 2.f, bi1 = b.x + b.z / 2.f, bj0 = b.y - b.w / 2.f, bj1 = b.y + b.w / 2.f;
    const float ih = fminf(ai1, bi1) - fmaxf(ai0, bi0), iw = fminf(aj1, bj1) - fmaxf(aj0, bj0);
    const float inter = (ih > 0.f ? ih : 0.f) * (iw > 0.f ? iw : 0.f);
    const float uni = a.z * a.w + b.z * b.w - inter;
    const float q = inter * __builtin_amdgcn_rcpf(uni);
    if (uni > 0.f && fabsf(q - thr) > 1e-6f && q <= 2.f) return q > thr;   // (q <= 2: its error stays below the margin)
    return (uni > 0.f ? inter / uni : 0.f) > thr;
}

}  // namespace d2t
