// Filling the frames between edited key frames along the source video's optical flow: an in-between frame t takes
// the edit of its previous and next key frame along the trajectories G of the SOURCE video, each side weighed by its distance in time,
// by whether the trajectory is visible (U, from the forward-backward rule of section 19) and by whether the source A looks the same at
// both of its ends.  include/insv2v_hip.h states the definition, tests/keyfill_ref.py restates it in float64.  The temporal filter's
// layout, for the same reason: one thread per pixel, consecutive lanes walk a row, so G, U, A_t and the stores are coalesced and the four
// taps of a smooth flow fall into neighbouring lines.  No reduction across threads, no read-modify-write: two calls give the same bits.
#include "common.h"
#include "flow_sample.h"
#include <math.h>
#include <vector>

namespace {

struct View {   // insv2v_frames_view by value
    const void* p;
    int64_t st, sc, sh;
    float scale, shift;
};
template <bool F32> __device__ __forceinline__ float ld(const void* p, int64_t off) {
    return F32 ? ((const float*)p)[off] : (float)((const half_t*)p)[off];
}
// the guide as it is read: clamp(x * scale + shift, 0, 1) of a raw value (a NaN stays a NaN)
__device__ __forceinline__ float guide(const View& v, float x) {
    const float a = x * v.scale + v.shift;
    return a != a ? a : fminf(fmaxf(a, 0.f), 1.f);
}
// The frame table of one launch, by value: per frame and side the key slot (-1: no such side), the key's frame of A, the temporal
// weight tw and tw renormalised over the existing sides.
struct Table {
    int32_t t[INSV2V_KEYFILL_MAX_FRAMES];
    int32_t slot[INSV2V_KEYFILL_MAX_FRAMES][2], key[INSV2V_KEYFILL_MAX_FRAMES][2];
    float tw[INSV2V_KEYFILL_MAX_FRAMES][2], twn[INSV2V_KEYFILL_MAX_FRAMES][2];
};

template <bool EF32, bool AF32>
__global__ __launch_bounds__(256) void keyfill_kernel(View a, View e, const float* __restrict__ flow, const float* __restrict__ valid,
                                                      void* __restrict__ out, int64_t ot, int64_t oc, int64_t oh, float* __restrict__ conf,
                                                      Table tab, int base, int H, int W, float neg_inv_2s2, int warp) {
    const int64_t plane = (int64_t)H * W;
    const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= plane) return;
    const int j = blockIdx.y;                 // the frame of this launch's table
    const int64_t i = (int64_t)base + j;      // ... and of flow / valid / conf
    const int t = tab.t[j];
    const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
    const int64_t a0 = (int64_t)t * a.st + (int64_t)y * a.sh + x;
    float ar[3], ag[3], num[3] = {0.f, 0.f, 0.f}, wsum = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) ar[c] = ld<AF32>(a.p, a0 + c * a.sc), ag[c] = guide(a, ar[c]);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const int slot = tab.slot[j][s];
        if (slot < 0) continue;                                                   // the side does not exist
        if (!(valid[(i * 2 + s) * plane + r] > 0.5f)) continue;                   // an invalid side is skipped, not multiplied by 0
        const float gx = flow[(i * 2 + s) * 2 * plane + r], gy = flow[((i * 2 + s) * 2 + 1) * plane + r];
        const MtTaps tp = mt_taps((float)x + gx, (float)y + gy, H, W);        // (clamped before it becomes an index)
        const int64_t ak = (int64_t)tab.key[j][s] * a.st, ek = (int64_t)slot * e.st;
        const int64_t ar0 = (int64_t)tp.y0 * a.sh, ar1 = (int64_t)tp.y1 * a.sh, er0 = (int64_t)tp.y0 * e.sh, er1 = (int64_t)tp.y1 * e.sh;
        float d2 = 0.f, res[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t oa = ak + c * a.sc, oe = ek + c * e.sc;
            const float a00 = ld<AF32>(a.p, oa + ar0 + tp.x0), a01 = ld<AF32>(a.p, oa + ar0 + tp.x1);
            const float a10 = ld<AF32>(a.p, oa + ar1 + tp.x0), a11 = ld<AF32>(a.p, oa + ar1 + tp.x1);
            const float e00 = ld<EF32>(e.p, oe + er0 + tp.x0), e01 = ld<EF32>(e.p, oe + er0 + tp.x1);
            const float e10 = ld<EF32>(e.p, oe + er1 + tp.x0), e11 = ld<EF32>(e.p, oe + er1 + tp.x1);
            const float d = ag[c] - mt_lerp(tp, guide(a, a00), guide(a, a01), guide(a, a10), guide(a, a11));
            d2 += d * d;
            res[c] = warp ? mt_lerp(tp, e00, e01, e10, e11) - ar[c] : mt_lerp(tp, e00 - a00, e01 - a01, e10 - a10, e11 - a11);
        }
        const float w = tab.tw[j][s] * expf((d2 / 3.f) * neg_inv_2s2);
#pragma unroll
        for (int c = 0; c < 3; ++c) num[c] += w * res[c];
        wsum += w;
    }
    float q[3];
    if (wsum > 0.f) {
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = num[c] / wsum;
    } else {   // a hole: no active side, or every weight underflowed - the temporal blend of the keys at x itself, no flow read
        wsum = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) q[c] = 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int slot = tab.slot[j][s];
            if (slot < 0) continue;
            const int64_t ak = (int64_t)tab.key[j][s] * a.st + (int64_t)y * a.sh + x, ek = (int64_t)slot * e.st + (int64_t)y * e.sh + x;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float ev = ld<EF32>(e.p, ek + c * e.sc);
                q[c] += tab.twn[j][s] * (warp ? ev - ar[c] : ev - ld<AF32>(a.p, ak + c * a.sc));
            }
        }
    }
    const int64_t o0 = (int64_t)t * ot + (int64_t)y * oh + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float v = q[c] == 0.f ? ar[c] : ar[c] + q[c];   // nothing to add leaves the source's bits (also those of a -0)
        if (EF32) ((float*)out)[o0 + c * oc] = v;
        else ((half_t*)out)[o0 + c * oc] = (half_t)v;
    }
    if (conf) conf[i * plane + r] = wsum;
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

extern "C" int insv2v_keyframe_fill(const insv2v_keyfill_desc* d, insv2v_stream_t stream) {
    if (!d || !d->flow || !d->valid || !d->out || !d->key_frame || !d->frame || !d->slot || !d->weight) return INSV2V_EINVAL;
    const int32_t n = d->n, T = d->T, Tk = d->Tk, H = d->H, W = d->W;
    if (n < 1 || T < 1 || Tk < 1 || H <= 1 || W <= 1 || H > MAX_SIDE || W > MAX_SIDE) return INSV2V_EINVAL;
    if (d->mode != INSV2V_KEYFILL_RESIDUAL && d->mode != INSV2V_KEYFILL_WARP) return INSV2V_EINVAL;
    if (!isfinite(d->sigma) || !(d->sigma > 0.f)) return INSV2V_EINVAL;
    if (!isfinite(d->a.scale) || !isfinite(d->a.shift)) return INSV2V_EINVAL;
    const int64_t plane = (int64_t)H * W;
    const int64_t blocks = (plane + 255) / 256;
    if (T > 65535 || Tk > 65535 || n > T || blocks > 0x7fffffffll) return INSV2V_EINVAL;
    if (plane > MAX_ELEMS / 4 / n) return INSV2V_EINVAL;         // n * 2 * 2 * H * W stays below MAX_ELEMS
    if (!strides_ok(d->a.p, d->a.stride_t, d->a.stride_c, d->a.stride_h, T, H, W) ||
        !strides_ok(d->e.p, d->e.stride_t, d->e.stride_c, d->e.stride_h, Tk, H, W) ||
        !strides_ok(d->out, d->out_stride_t, d->out_stride_c, d->out_stride_h, T, H, W))
        return INSV2V_EINVAL;
    const double s2 = 2.0 * (double)d->sigma * (double)d->sigma;
    const float neg_inv_2s2 = (float)(-1.0 / s2);
    if (!(s2 > 0.0) || !isfinite(neg_inv_2s2)) return INSV2V_EINVAL;   // (a sigma so small that its square underflows)
    // the tables: every frame once, none of them a key frame, every slot a key, the weights of the existing sides a partition of 1
    std::vector<uint8_t> seen((size_t)T, 0);   // 1 = a key frame, 2 = a frame of the table
    for (int j = 0; j < Tk; ++j) {
        if (d->key_frame[j] < 0 || d->key_frame[j] >= T) return INSV2V_EINVAL;
        seen[d->key_frame[j]] = 1;
    }
    for (int i = 0; i < n; ++i) {
        const int32_t t = d->frame[i];
        if (t < 0 || t >= T || seen[t]) return INSV2V_EINVAL;
        seen[t] = 2;
        double sum = 0.0;
        int sides = 0;
        for (int s = 0; s < 2; ++s) {
            const int32_t slot = d->slot[2 * i + s];
            const float tw = d->weight[2 * i + s];
            if (slot < -1 || slot >= Tk || !isfinite(tw) || tw < 0.f) return INSV2V_EINVAL;
            if (slot >= 0) sum += (double)tw, ++sides;
        }
        if (!sides || !(fabs(sum - 1.0) <= 1e-6)) return INSV2V_EINVAL;
    }
    // A pixel reads other frames; the output and conf may overlap no input and not each other.
    const int esz = d->e.fp32 ? 4 : 2;
    const Span o = span_of(d->out, d->out_stride_t, d->out_stride_c, d->out_stride_h, T, H, W, esz);
    const Span cf{(uintptr_t)d->conf, d->conf ? (uintptr_t)((int64_t)n * plane * 4) : 0};
    const Span in[4] = {span_of(d->e.p, d->e.stride_t, d->e.stride_c, d->e.stride_h, Tk, H, W, esz),
                        span_of(d->a.p, d->a.stride_t, d->a.stride_c, d->a.stride_h, T, H, W, d->a.fp32 ? 4 : 2),
                        Span{(uintptr_t)d->flow, (uintptr_t)((int64_t)n * 4 * plane * 4)},
                        Span{(uintptr_t)d->valid, (uintptr_t)((int64_t)n * 2 * plane * 4)}};
    for (int i = 0; i < 4; ++i)
        if (overlap(o, in[i]) || overlap(cf, in[i])) return INSV2V_EINVAL;
    if (overlap(o, cf)) return INSV2V_EINVAL;
    const View a{d->a.p, d->a.stride_t, d->a.stride_c, d->a.stride_h, d->a.scale, d->a.shift};
    const View e{d->e.p, d->e.stride_t, d->e.stride_c, d->e.stride_h, 1.f, 0.f};
    auto kern = d->e.fp32 ? (d->a.fp32 ? keyfill_kernel<true, true> : keyfill_kernel<true, false>)
                          : (d->a.fp32 ? keyfill_kernel<false, true> : keyfill_kernel<false, false>);
    for (int base = 0; base < n; base += INSV2V_KEYFILL_MAX_FRAMES) {
        const int m = n - base < INSV2V_KEYFILL_MAX_FRAMES ? n - base : INSV2V_KEYFILL_MAX_FRAMES;
        Table tab = {};
        for (int j = 0; j < m; ++j) {
            const int i = base + j;
            tab.t[j] = d->frame[i];
            double sum = 0.0;
            for (int s = 0; s < 2; ++s)
                if (d->slot[2 * i + s] >= 0) sum += (double)d->weight[2 * i + s];
            for (int s = 0; s < 2; ++s) {
                const int32_t slot = d->slot[2 * i + s];
                tab.slot[j][s] = slot;
                tab.key[j][s] = slot >= 0 ? d->key_frame[slot] : 0;
                tab.tw[j][s] = slot >= 0 ? d->weight[2 * i + s] : 0.f;
                tab.twn[j][s] = slot >= 0 ? (float)((double)d->weight[2 * i + s] / sum) : 0.f;
            }
        }
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks, (unsigned)m), dim3(256), 0, as_stream(stream), a, e, d->flow, d->valid, d->out,
                           d->out_stride_t, d->out_stride_c, d->out_stride_h, d->conf, tab, base, (int)H, (int)W, neg_inv_2s2,
                           (int)(d->mode == INSV2V_KEYFILL_WARP));
        const int rc = launch_status();
        if (rc) return rc;
    }
    return 0;
}
