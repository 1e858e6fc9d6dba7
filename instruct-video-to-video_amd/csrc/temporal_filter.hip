// Stabilizing an edit along the source video's optical flow: every pixel of the edit E is averaged with its
// neighbours in time along the trajectories G of the SOURCE video, each neighbour weighed by whether the trajectory is visible (U, from
// the forward-backward rule of section 19) and by whether the source A looks the same at both of its ends.  include/insv2v_hip.h states
// the definition, tests/temporal_filter_ref.py restates it in float64.  A gather over a few planes: one thread per pixel, consecutive
// lanes walk a row, so G, U, E_t, A_t and the stores are coalesced and the four taps of a smooth flow fall into neighbouring lines.
// No reduction across threads, no read-modify-write on global memory: two calls give the same bits.
#include "common.h"
#include "flow_sample.h"
#include <math.h>

namespace {

struct View {   // insv2v_frames_view by value
    const void* p;
    int64_t st, sc, sh;
    float scale, shift;
};
template <bool F32> __device__ __forceinline__ float ld(const void* p, int64_t off) {
    return F32 ? ((const float*)p)[off] : (float)((const half_t*)p)[off];
}
// the guide as it is read: clamp(x * scale + shift, 0, 1) (a NaN stays a NaN)
template <bool F32> __device__ __forceinline__ float rd(const View& v, int64_t off) {
    const float a = ld<F32>(v.p, off) * v.scale + v.shift;
    return a != a ? a : fminf(fmaxf(a, 0.f), 1.f);
}
struct Offsets { int32_t k[INSV2V_TFILTER_MAX_K]; };

template <bool EF32, bool AF32>
__global__ __launch_bounds__(256) void temporal_filter_kernel(View e, View a, const float* __restrict__ flow, const float* __restrict__ valid,
                                                              void* __restrict__ out, int64_t ot, int64_t oc, int64_t oh, Offsets offs,
                                                              int K, int T, int H, int W, float neg_inv_2s2, float strength) {
    const int64_t plane = (int64_t)H * W;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= plane) return;
    const int t = blockIdx.y;
    const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
    const int64_t e0 = (int64_t)t * e.st + (int64_t)y * e.sh + x, a0 = (int64_t)t * a.st + (int64_t)y * a.sh + x;
    float ec[3], ac[3], num[3] = {0.f, 0.f, 0.f}, den = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) ec[c] = ld<EF32>(e.p, e0 + c * e.sc), ac[c] = rd<AF32>(a, a0 + c * a.sc);
    for (int k = 0; k < K; ++k) {
        const int tn = t + offs.k[k];
        if (tn < 0 || tn >= T) continue;                                      // outside the video: skipped whatever U holds there
        const int64_t kt = (int64_t)k * T + t;
        if (!(valid[kt * plane + r] > 0.5f)) continue;                        // an invalid neighbour is skipped, not multiplied by 0
        const float gx = flow[kt * 2 * plane + r], gy = flow[(kt * 2 + 1) * plane + r];
        const MtTaps tp = mt_taps((float)x + gx, (float)y + gy, H, W);    // (clamped before it becomes an index)
        const int64_t r0 = (int64_t)tp.y0, r1 = (int64_t)tp.y1;
        const int64_t an = (int64_t)tn * a.st, en = (int64_t)tn * e.st;
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t o = an + c * a.sc;
            const float g = mt_lerp(tp, rd<AF32>(a, o + r0 * a.sh + tp.x0), rd<AF32>(a, o + r0 * a.sh + tp.x1),
                                    rd<AF32>(a, o + r1 * a.sh + tp.x0), rd<AF32>(a, o + r1 * a.sh + tp.x1));
            const float d = ac[c] - g;
            s += d * d;
        }
        const float w = strength * expf((s / 3.f) * neg_inv_2s2);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t o = en + c * e.sc;
            const float g = mt_lerp(tp, ld<EF32>(e.p, o + r0 * e.sh + tp.x0), ld<EF32>(e.p, o + r0 * e.sh + tp.x1),
                                    ld<EF32>(e.p, o + r1 * e.sh + tp.x0), ld<EF32>(e.p, o + r1 * e.sh + tp.x1));
            num[c] += w * (g - ec[c]);
        }
        den += w;
    }
    const float inv = 1.f + den;
    const int64_t o0 = (int64_t)t * ot + (int64_t)y * oh + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float q = num[c] / inv;
        const float v = q == 0.f ? ec[c] : ec[c] + q;   // the residual form: nothing to add leaves E's bits (also those of a -0)
        if (EF32) ((float*)out)[o0 + c * oc] = v;
        else ((half_t*)out)[o0 + c * oc] = (half_t)v;
    }
}

// ------------------------------------------------------------------------------------------------------------------ host side
struct Span {
    uintptr_t lo, n;
};
bool overlap(const Span& a, const Span& b) { return a.n && b.n && a.lo < b.lo + b.n && b.lo < a.lo + a.n; }
constexpr int64_t MAX_SIDE = 1 << 24;             // pixel coordinates are exact in fp32
constexpr int64_t MAX_ELEMS = (int64_t)1 << 40;   // of any operand: no offset or byte count overflows int64
bool strides_ok(const void* p, int64_t st, int64_t sc, int64_t sh, int32_t T, int32_t H, int32_t W) {
    if (!p || st < 0 || sc < 0 || sh < W) return false;
    return st <= MAX_ELEMS / T && sc <= MAX_ELEMS / 3 && sh <= MAX_ELEMS / H;
}
Span span_of(const void* p, int64_t st, int64_t sc, int64_t sh, int32_t T, int32_t H, int32_t W, int elem) {
    const int64_t elems = (int64_t)(T - 1) * st + 2 * sc + (int64_t)(H - 1) * sh + W;
    return Span{(uintptr_t)p, (uintptr_t)(elems * elem)};
}

}   // namespace

extern "C" int insv2v_temporal_filter(const insv2v_temporal_filter_desc* d, insv2v_stream_t stream) {
    if (!d || !d->flow || !d->valid || !d->out) return INSV2V_EINVAL;
    const int32_t T = d->T, H = d->H, W = d->W, K = d->K;
    if (T < 1 || H <= 1 || W <= 1 || H > MAX_SIDE || W > MAX_SIDE || K < 1 || K > INSV2V_TFILTER_MAX_K) return INSV2V_EINVAL;
    for (int k = 0; k < K; ++k)
        if (d->offsets[k] == 0 || d->offsets[k] < -INSV2V_TFILTER_MAX_RADIUS || d->offsets[k] > INSV2V_TFILTER_MAX_RADIUS) return INSV2V_EINVAL;
    if (!isfinite(d->sigma) || !(d->sigma > 0.f) || !(d->strength > 0.f) || !(d->strength <= 1.f)) return INSV2V_EINVAL;
    if (!isfinite(d->a.scale) || !isfinite(d->a.shift)) return INSV2V_EINVAL;
    const int64_t plane = (int64_t)H * W;
    if (plane > MAX_ELEMS / 8 / T / 2) return INSV2V_EINVAL;     // K * T * 2 * H * W stays below MAX_ELEMS
    if (!strides_ok(d->e.p, d->e.stride_t, d->e.stride_c, d->e.stride_h, T, H, W) ||
        !strides_ok(d->a.p, d->a.stride_t, d->a.stride_c, d->a.stride_h, T, H, W) ||
        !strides_ok(d->out, d->out_stride_t, d->out_stride_c, d->out_stride_h, T, H, W))
        return INSV2V_EINVAL;
    const double s2 = 2.0 * (double)d->sigma * (double)d->sigma;
    const float neg_inv_2s2 = (float)(-1.0 / s2);
    if (!(s2 > 0.0) || !isfinite(neg_inv_2s2)) return INSV2V_EINVAL;   // (a sigma so small that its square underflows)
    const int64_t blocks = (plane + 255) / 256;
    if (T > 65535 || blocks > 0x7fffffffll) return INSV2V_EINVAL;
    // A pixel reads other frames that other threads write: the output may overlap no input.
    const int esz = d->e.fp32 ? 4 : 2;
    const Span o = span_of(d->out, d->out_stride_t, d->out_stride_c, d->out_stride_h, T, H, W, esz);
    const Span in[4] = {span_of(d->e.p, d->e.stride_t, d->e.stride_c, d->e.stride_h, T, H, W, esz),
                        span_of(d->a.p, d->a.stride_t, d->a.stride_c, d->a.stride_h, T, H, W, d->a.fp32 ? 4 : 2),
                        Span{(uintptr_t)d->flow, (uintptr_t)((int64_t)K * T * 2 * plane * 4)},
                        Span{(uintptr_t)d->valid, (uintptr_t)((int64_t)K * T * plane * 4)}};
    for (int i = 0; i < 4; ++i)
        if (overlap(o, in[i])) return INSV2V_EINVAL;
    Offsets offs;
    for (int k = 0; k < INSV2V_TFILTER_MAX_K; ++k) offs.k[k] = k < K ? d->offsets[k] : 0;
    const View e{d->e.p, d->e.stride_t, d->e.stride_c, d->e.stride_h, 1.f, 0.f};
    const View a{d->a.p, d->a.stride_t, d->a.stride_c, d->a.stride_h, d->a.scale, d->a.shift};
    auto kern = d->e.fp32 ? (d->a.fp32 ? temporal_filter_kernel<true, true> : temporal_filter_kernel<true, false>)
                          : (d->a.fp32 ? temporal_filter_kernel<false, true> : temporal_filter_kernel<false, false>);
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)T), dim3(256), 0, as_stream(stream), e, a, d->flow, d->valid, d->out,
                       d->out_stride_t, d->out_stride_c, d->out_stride_h, offs, (int)K, (int)T, (int)H, (int)W, neg_inv_2s2, d->strength);
    return launch_status();
}
