// Sampling a plane along an optical flow, and the forward-backward consistency rule: ONE copy, shared by the key-frame mask chain
// (masktrack.hip) and the flow warp error (pixel_score.hip), so the two cannot drift apart (include/insv2v_hip.h, insv2v_mask_track_step,
// states the definition; tests/masktrack_ref.py restates it in float64).
#pragma once
#include "common.h"

// Border-clamped bilinear sample at a point: the point is clamped to the frame, x0 = floor, x1 = min(x0 + 1, W - 1), the same in y.
// (A NaN coordinate clamps to 0: fmaxf returns its other operand.  The integer clamp covers a W - 1 that fp32 rounds up.)
// Evaluated as lerps - top + ay (bottom - top), top = g00 + ax (g01 - g00) - so a constant region is sampled exactly: a binary mask
// stays exactly 0 / 1 away from its edges.  A tap's bilinear weight is non-zero iff its ax / ay factors are (ax, ay in [0, 1)).
struct MtTaps {
    int64_t o00, o01, o10, o11;   // offsets into a contiguous [H,W] plane
    int x0, x1, y0, y1;           // the same taps as indices, for a plane with a row stride of its own
    float ax, ay;
};
__device__ __forceinline__ MtTaps mt_taps(float px, float py, int H, int W) {
    const float cx = fminf(fmaxf(px, 0.f), (float)(W - 1)), cy = fminf(fmaxf(py, 0.f), (float)(H - 1));
    const float fx = floorf(cx), fy = floorf(cy);
    const int x0 = min(max((int)fx, 0), W - 1), y0 = min(max((int)fy, 0), H - 1);
    const int x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1);
    MtTaps t;
    t.ax = cx - fx, t.ay = cy - fy;
    t.x0 = x0, t.x1 = x1, t.y0 = y0, t.y1 = y1;
    t.o00 = (int64_t)y0 * W + x0, t.o01 = (int64_t)y0 * W + x1, t.o10 = (int64_t)y1 * W + x0, t.o11 = (int64_t)y1 * W + x1;
    return t;
}
__device__ __forceinline__ float mt_lerp(const MtTaps& t, float g00, float g01, float g10, float g11) {
    const float top = g00 + t.ax * (g01 - g00), bottom = g10 + t.ax * (g11 - g10);
    return top + t.ay * (bottom - top);
}
__device__ __forceinline__ float mt_sample(const MtTaps& t, const float* __restrict__ g) {
    return mt_lerp(t, g[t.o00], g[t.o01], g[t.o10], g[t.o11]);
}
// p = x + b inside the frame (false for NaN)
__device__ __forceinline__ bool mt_inb(float px, float py, int H, int W) {
    return px >= 0.f && px <= (float)(W - 1) && py >= 0.f && py <= (float)(H - 1);
}
// The forward-backward consistency of b with the opposite flow cf sampled where b points: |b + cf|^2 <= alpha (|b|^2 + |cf|^2) + beta.
__device__ __forceinline__ bool mt_consistent(float bx, float by, float cfx, float cfy, float alpha, float beta) {
    const float dx = bx + cfx, dy = by + cfy;
    return dx * dx + dy * dy <= alpha * ((bx * bx + by * by) + (cfx * cfx + cfy * cfy)) + beta;
}
