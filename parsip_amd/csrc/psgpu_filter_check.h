// psgpu_filter_check.h — what psgpu_weld_filter accepts of its arguments (host only, no HIP:
// tests/cpp/filter_args_check.cpp runs it under the host sanitizers).
#pragma once
#include <cmath>

#include "../../include/parsip_gpu.h"

namespace psgpu {

// The criteria of a filter call as the kernels take them: the caller's, or all zero for NULL.
// false: an unknown flag bit, reserved != 0, or a threshold that is NaN, infinite or negative.
inline bool filter_criteria(const PsShellFilter* f, PsShellFilter* out) {
    PsShellFilter c{};
    if (f) c = *f;
    *out = c;
    if (c.flags & ~(uint32_t)(PSGPU_FILTER_CLOSED_ONLY | PSGPU_FILTER_DROP_CAVITIES)) return false;
    if (c.reserved != 0) return false;
    if (!std::isfinite(c.minArea) || !std::isfinite(c.minAbsVolume)) return false;
    return c.minArea >= 0.0 && c.minAbsVolume >= 0.0;
}

// The mask of a filter call over ctShells shells: none, or one byte per shell.
inline bool filter_mask_fits(const uint8_t* mask, uint32_t maskCount, uint32_t ctShells) {
    return mask == nullptr || maskCount == ctShells;
}

}  // namespace psgpu
