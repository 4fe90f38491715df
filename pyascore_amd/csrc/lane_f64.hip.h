/* lane_f64.hip.h -- what markers.hip and purity.hip share: a double held by one lane, to every lane, through scalar registers. */
#pragma once
#include "device_common.hip.h"

/* a double held by lane `src` (wave-uniform), to every lane: two v_readlane */
DEV double marker_lane_f64(double v, int src) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, src);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), src);
    return __longlong_as_double((long long)(((uint64_t)hi << 32) | (uint64_t)lo));
}
