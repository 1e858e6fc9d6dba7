// What insv2v_mask_shape does with (grow, feather) as a pure function: plan_mask_shape -> insv2v_mask_shape_plan_t.
// Host-only, no HIP call, no static, no environment read.  insv2v_mask_shape validates through it, then launches what it says;
// insv2v_mask_shape_plan returns it without touching a GPU.  include/insv2v_hip.h states the definition.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/insv2v_hip.h"

constexpr int MASK_SHAPE_ROW_TILE = 256;   // pixels of a row one workgroup of the row pass owns (mask_shape.hip: one per thread)

// The four thresholds are the float64 decisions on s themselves, turned into integers: sqrt of an integer is monotone, also after its
// rounding, so "the largest N with sqrt(N) <= g" read off a scan of 0 .. FAR decides every D2 exactly as the comparison on s would.
// (floor(g^2) and ceil((g+f)^2) are the same numbers wherever the squares are exact in double; the scan has no such condition.)
static inline insv2v_mask_shape_plan_t plan_mask_shape(float grow, float feather) {
    insv2v_mask_shape_plan_t p = {};
    p.rc = INSV2V_EINVAL;
    p.row_tile = MASK_SHAPE_ROW_TILE;
    if (!isfinite(grow) || !isfinite(feather)) return p;
    const double g = (double)grow, f = (double)feather, h = g + f;
    if (g < -INSV2V_MASK_SHAPE_MAX || g > INSV2V_MASK_SHAPE_MAX || f < 0.0 || f > INSV2V_MASK_SHAPE_MAX || h < -INSV2V_MASK_SHAPE_MAX) return p;
    const double reach = fmax(fmax(h, 1.0 - g), 1.0);
    p.R = (int32_t)ceil(reach);
    p.far = (p.R + 1) * (p.R + 1);
    p.out_one = -1, p.in_zero = -1, p.out_zero = p.far, p.in_one = p.far;
    for (int32_t n = p.far; n >= 0; --n) {
        const double r = sqrt((double)n);
        if (r >= h) p.out_zero = n;            // the smallest n with  sqrt(n) >= g + f
        if (1.0 - r <= g) p.in_one = n;        // the smallest n with  1 - sqrt(n) <= g
    }
    for (int32_t n = 0; n <= p.far; ++n) {
        const double r = sqrt((double)n);
        if (r <= g) p.out_one = n;             // the largest n with  sqrt(n) <= g
        if (1.0 - r >= h) p.in_zero = n;       // the largest n with  1 - sqrt(n) >= g + f
    }
    p.rc = 0;
    return p;
}
