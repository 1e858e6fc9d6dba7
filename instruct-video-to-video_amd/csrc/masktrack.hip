// Tracking a key-frame mask through the video with optical flow: one step of the chain that carries the flow to
// the key frame, its validity and the tracked mask from a frame t' to its neighbour t.  tests/masktrack_ref.py restates the definition in
// float64.  A gather over a few fp32 planes: launch-bound at video sizes, no matrix cores, nothing tuned beyond row-major access.
#include "common.h"
#include "flow_sample.h"
#include <math.h>

// The border-clamped bilinear sample (mt_taps / mt_sample) and the consistency rule (mt_consistent) live in flow_sample.h, shared with
// the flow warp error of pixel_score.hip.
// One thread per pixel (n, y, x) of the N chains; consecutive threads walk a row, so b, c's centre and every store are coalesced.
__global__ __launch_bounds__(256) void mask_track_step_kernel(const float* __restrict__ f_prev, const float* __restrict__ v_prev,
                                                              const float* __restrict__ b, const float* __restrict__ c,
                                                              const float* __restrict__ m, float* __restrict__ f_out,
                                                              float* __restrict__ v_out, float* __restrict__ mask_out, int64_t total,
                                                              int H, int W, float alpha, float beta, float fill) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over [N,H,W]
    if (i >= total) return;
    const int64_t plane = (int64_t)H * W;
    const int64_t n = i / plane, r = i - n * plane;
    const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
    const float bx = b[n * 2 * plane + r], by = b[(n * 2 + 1) * plane + r];
    const float px = (float)x + bx, py = (float)y + by;
    const bool inb = px >= 0.f && px <= (float)(W - 1) && py >= 0.f && py <= (float)(H - 1);   // (false for NaN)
    const MtTaps t = mt_taps(px, py, H, W);
    bool cons = true;
    if (c) {
        const float cfx = mt_sample(t, c + n * 2 * plane), cfy = mt_sample(t, c + (n * 2 + 1) * plane);
        cons = mt_consistent(bx, by, cfx, cfy, alpha, beta);
    }
    const float* vp = v_prev + n * plane;
    float vs = fminf(1.f, vp[t.o00]);
    if (t.ax != 0.f) vs = fminf(vs, vp[t.o01]);
    if (t.ay != 0.f) vs = fminf(vs, vp[t.o10]);
    if (t.ax != 0.f && t.ay != 0.f) vs = fminf(vs, vp[t.o11]);
    const float fx = bx + mt_sample(t, f_prev + n * 2 * plane), fy = by + mt_sample(t, f_prev + (n * 2 + 1) * plane);
    const bool valid = inb && cons && vs > 0.5f;
    f_out[n * 2 * plane + r] = fx;
    f_out[(n * 2 + 1) * plane + r] = fy;
    v_out[i] = valid ? 1.f : 0.f;
    float mv = fill;
    if (valid) mv = mt_sample(mt_taps((float)x + fx, (float)y + fy, H, W), m + n * plane);
    mask_out[i] = mv;
}

extern "C" int insv2v_mask_track_step(const insv2v_masktrack_desc* d, insv2v_stream_t stream) {
    if (!d || !d->f_prev || !d->v_prev || !d->b || !d->m || !d->f_out || !d->v_out || !d->mask_out) return INSV2V_EINVAL;   // (c may be NULL)
    if (d->N <= 0 || d->H <= 1 || d->W <= 1) return INSV2V_EINVAL;
    if (!(d->alpha >= 0.f) || !(d->beta >= 0.f) || !isfinite(d->alpha) || !isfinite(d->beta) || isnan(d->fill)) return INSV2V_EINVAL;
    const int64_t plane = (int64_t)d->H * d->W;
    if (plane > INT64_MAX / 8 / d->N) return INSV2V_EINVAL;
    const int64_t total = (int64_t)d->N * plane;
    if ((2 * total + 255) / 256 > 0x7fffffffll) return INSV2V_EINVAL;
    // A pixel reads neighbours that other threads write: no output may overlap an input, or another output.
    const uintptr_t one = (uintptr_t)total * sizeof(float), two = 2 * one;
    auto overlap = [](const void* a, uintptr_t na, const void* b, uintptr_t nb) {
        return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
    };
    const void* in[5] = {d->f_prev, d->v_prev, d->b, d->c, d->m};
    const uintptr_t in_bytes[5] = {two, one, two, two, one};
    const void* out[3] = {d->f_out, d->v_out, d->mask_out};
    const uintptr_t out_bytes[3] = {two, one, one};
    for (int o = 0; o < 3; ++o) {
        for (int k = 0; k < 5; ++k)
            if (in[k] && overlap(out[o], out_bytes[o], in[k], in_bytes[k])) return INSV2V_EINVAL;
        for (int p = 0; p < o; ++p)
            if (overlap(out[o], out_bytes[o], out[p], out_bytes[p])) return INSV2V_EINVAL;
    }
    const int64_t grid = (total + 255) / 256;
    hipLaunchKernelGGL(mask_track_step_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), d->f_prev, d->v_prev, d->b, d->c, d->m,
                       d->f_out, d->v_out, d->mask_out, total, (int)d->H, (int)d->W, d->alpha, d->beta, d->fill);
    return launch_status();
}
