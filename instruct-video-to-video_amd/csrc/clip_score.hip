// Scoring an edit with CLIP (reference: ClipSimilarity, misc_utils/clip_similarity.py:10-47): the two kernels of the metric that are
// not a GEMM, a LayerNorm or an attention.
//
//   insv2v_clip_preprocess   encode_image's pixel front end (:29-31) in one pass: bicubic resample of the frame to S x S, the CLIP
//                            mean / std normalisation, and the im2col of the non-overlapping P x P patches, so that the patch
//                            embedding (a stride-P convolution without bias) is a plain insv2v_gemm over the rows written here.
//   insv2v_clip_scores       :25,:33,:43-46 plus the frame-consistency cosine of the LOVEU-TGVE benchmark, from the towers' features.
//
// Both run once per scored clip next to 59 TFLOP of denoising per frame: written for exactness and coalesced stores, not for speed.
#include "common.h"

// ---- bicubic (A = -0.75, align_corners = False, no antialias) + normalise + patch rows ----------------------------------------------
// torch's upsample_bicubic2d: the source coordinate (dst + 0.5) * in / out - 0.5 is NOT clamped, the four tap indices are.
// The coordinate is the rational ((2 dst + 1) in - out) / (2 out): its floor and fraction are taken in integers, so the fraction is rounded
// once.  (Evaluated in fp32 the coordinate carries half an ulp of a number up to `in` - 4e-6 at 64 rows - and the weights' slope turns
// that into 2e-5 of a normalised pixel: measured, and the same size as the error of torch's own fp32 kernel against float64.)
__device__ __forceinline__ int source_coord(int dst, int in, int out, float* frac) {
    const int64_t num = (int64_t)(2 * dst + 1) * in - out, den = 2 * (int64_t)out;
    int64_t q = num / den, r = num - q * den;
    if (r < 0) { r += den; q -= 1; }
    *frac = (float)r / (float)den;
    return (int)q;
}
__device__ __forceinline__ void cubic_weights(float t, float w[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.f, x3 = 2.f - t, x2 = 1.f - t;
    w[0] = ((A * x0 - 5.f * A) * x0 + 8.f * A) * x0 - 4.f * A;
    w[1] = ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    w[2] = ((A + 2.f) * x2 - (A + 3.f)) * x2 * x2 + 1.f;
    w[3] = ((A * x3 - 5.f * A) * x3 + 8.f * A) * x3 - 4.f * A;
}

struct clip_pre_params {
    const void* x;
    half_t* out;
    int64_t sn, sc, sh, sw, ld, total;
    int H, W, S, P;
    float in_scale, in_shift;
    float mean[3], rstd[3];
};

template <typename T>
__global__ __launch_bounds__(256) void clip_preprocess_kernel(const clip_pre_params p) {
    const T* x = (const T*)p.x;
    const int G = p.S / p.P, PP = p.P * p.P, cols = 3 * PP;
    // consecutive lanes = consecutive columns of one patch row: coalesced stores; the 4 x 4 taps of neighbouring lanes overlap in the cache
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < p.total; idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = idx / p.ld;
        const int col = (int)(idx - row * p.ld);
        if (col >= cols) { p.out[idx] = (half_t)0.f; continue; }   // the pad columns of the GEMM's K: exact zeros
        const int c = col / PP, r = col - c * PP, py = r / p.P, px = r - py * p.P;
        const int gx = (int)(row % G), t = (int)(row / G), gy = t % G, img = t / G;
        const int oy = gy * p.P + py, ox = gx * p.P + px;
        float ty, tx, wy[4], wx[4];
        const int iy = source_coord(oy, p.H, p.S, &ty), ix = source_coord(ox, p.W, p.S, &tx);
        cubic_weights(ty, wy);
        cubic_weights(tx, wx);
        const T* base = x + (int64_t)img * p.sn + (int64_t)c * p.sc;
        int64_t xo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xo[j] = (int64_t)min(max(ix - 1 + j, 0), p.W - 1) * p.sw;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const T* rowp = base + (int64_t)min(max(iy - 1 + i, 0), p.H - 1) * p.sh;
            float h = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) h += wx[j] * (float)rowp[xo[j]];
            acc += wy[i] * h;
        }
        // the weights sum to one, so the affine map to [0, 1] commutes with the resample; the cubic's overshoot is kept (no clamp)
        const float v = (acc * p.in_scale + p.in_shift - p.mean[c]) * p.rstd[c];
        p.out[idx] = (half_t)v;
    }
}

extern "C" int insv2v_clip_preprocess(const insv2v_clip_preprocess_desc* dp, insv2v_stream_t stream) {
    if (!one_device() || !dp || !dp->x || !dp->out) return INSV2V_EINVAL;
    const insv2v_clip_preprocess_desc d = *dp;
    if (d.n <= 0 || d.H <= 0 || d.W <= 0 || d.S <= 0 || d.P <= 0 || d.S % d.P) return INSV2V_EINVAL;
    if (d.ld < (int64_t)3 * d.P * d.P) return INSV2V_EINVAL;
    for (int c = 0; c < 3; ++c)
        if (!(d.std[c] > 0.f)) return INSV2V_EINVAL;
    clip_pre_params p;
    p.x = d.x; p.out = (half_t*)d.out;
    p.sn = d.stride_n; p.sc = d.stride_c; p.sh = d.stride_h; p.sw = d.stride_w; p.ld = d.ld;
    const int64_t G = d.S / d.P;
    p.total = (int64_t)d.n * G * G * d.ld;
    p.H = d.H; p.W = d.W; p.S = d.S; p.P = d.P;
    p.in_scale = d.in_scale; p.in_shift = d.in_shift;
    for (int c = 0; c < 3; ++c) { p.mean[c] = d.mean[c]; p.rstd[c] = 1.0f / d.std[c]; }
    const int64_t want = (p.total + 255) / 256;
    const int blocks = (int)(want < 65536 * 4 ? want : 65536 * 4);
    if (d.x_fp32) hipLaunchKernelGGL(clip_preprocess_kernel<float>, dim3(blocks), dim3(256), 0, as_stream(stream), p);
    else hipLaunchKernelGGL(clip_preprocess_kernel<half_t>, dim3(blocks), dim3(256), 0, as_stream(stream), p);
    return launch_status();
}

// ---- the metrics ----------------------------------------------------------------------------------------------------------------------
// One wave per frame.  Every sum is taken by lane l over elements l, l + 64, ... in rising order and folded by the xor butterfly: a fixed
// order, so two calls give the same bits.  Pass 1: the five norms of encode_image / encode_text (:25, :33; no eps there).  Pass 2, on the
// normalised vectors: the dot products and the norms F.cosine_similarity takes itself (each clamped to eps on its own: ATen's
// cosine_similarity divides x1 by max(|x1|, eps) and x2 by max(|x2|, eps) before the dot).
template <typename T>
__global__ __launch_bounds__(64) void clip_scores_kernel(const T* img0, const T* img1, const T* txt0, const T* txt1, int64_t ld0, int64_t ld1,
                                                         int64_t ldt, int n, int D, float eps, float* out) {
    const int i = blockIdx.x, lane = threadIdx.x;
    const bool has_next = i + 1 < n;
    const T* a = img0 + (int64_t)i * ld0;
    const T* b = img1 + (int64_t)i * ld1;
    const T* c = img1 + (int64_t)(has_next ? i + 1 : i) * ld1;
    const T* s = txt0 + (int64_t)i * ldt;
    const T* t = txt1 + (int64_t)i * ldt;
    float na = 0.f, nb = 0.f, nc = 0.f, ns = 0.f, nt = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float va = (float)a[k], vb = (float)b[k], vc = (float)c[k], vs = (float)s[k], vt = (float)t[k];
        na += va * va; nb += vb * vb; nc += vc * vc; ns += vs * vs; nt += vt * vt;
    }
    na = sqrtf(wave_sum(na)); nb = sqrtf(wave_sum(nb)); nc = sqrtf(wave_sum(nc)); ns = sqrtf(wave_sum(ns)); nt = sqrtf(wave_sum(nt));
    float as = 0.f, bt = 0.f, ab = 0.f, bc = 0.f, de = 0.f, aa = 0.f, bb = 0.f, cc = 0.f, ss = 0.f, tt = 0.f, dd = 0.f, ee = 0.f;
    for (int k = lane; k < D; k += 64) {
        const float va = (float)a[k] / na, vb = (float)b[k] / nb, vc = (float)c[k] / nc, vs = (float)s[k] / ns, vt = (float)t[k] / nt;
        const float vd = vb - va, ve = vt - vs;
        as += va * vs; bt += vb * vt; ab += va * vb; bc += vb * vc; de += vd * ve;
        aa += va * va; bb += vb * vb; cc += vc * vc; ss += vs * vs; tt += vt * vt; dd += vd * vd; ee += ve * ve;
    }
    as = wave_sum(as); bt = wave_sum(bt); ab = wave_sum(ab); bc = wave_sum(bc); de = wave_sum(de);
    aa = fmaxf(sqrtf(wave_sum(aa)), eps); bb = fmaxf(sqrtf(wave_sum(bb)), eps); cc = fmaxf(sqrtf(wave_sum(cc)), eps);
    ss = fmaxf(sqrtf(wave_sum(ss)), eps); tt = fmaxf(sqrtf(wave_sum(tt)), eps);
    dd = fmaxf(sqrtf(wave_sum(dd)), eps); ee = fmaxf(sqrtf(wave_sum(ee)), eps);
    if (lane == 0) {
        float* o = out + (int64_t)i * 5;
        o[0] = as / (aa * ss);
        o[1] = bt / (bb * tt);
        o[2] = de / (dd * ee);
        o[3] = ab / (aa * bb);
        o[4] = has_next ? bc / (bb * cc) : 0.f;
    }
}

extern "C" int insv2v_clip_scores(const void* img0, const void* img1, const void* txt0, const void* txt1, int32_t fp32, int64_t ld0,
                                  int64_t ld1, int64_t ldt, int32_t n, int32_t D, float eps, float* out, insv2v_stream_t stream) {
    if (!one_device() || !img0 || !img1 || !txt0 || !txt1 || !out) return INSV2V_EINVAL;
    if (n <= 0 || D <= 0 || ld0 < D || ld1 < D || (ldt != 0 && ldt < D) || !(eps > 0.f)) return INSV2V_EINVAL;
    if (fp32)
        hipLaunchKernelGGL(clip_scores_kernel<float>, dim3(n), dim3(64), 0, as_stream(stream), (const float*)img0, (const float*)img1,
                           (const float*)txt0, (const float*)txt1, ld0, ld1, ldt, n, D, eps, out);
    else
        hipLaunchKernelGGL(clip_scores_kernel<half_t>, dim3(n), dim3(64), 0, as_stream(stream), (const half_t*)img0, (const half_t*)img1,
                           (const half_t*)txt0, (const half_t*)txt1, ld0, ld1, ldt, n, D, eps, out);
    return launch_status();
}

// ---- encode_image / encode_text's own last line (:25, :33): out = x / |x| per row, fp32 out, no eps (as the reference) -----------------
template <typename T>
__global__ __launch_bounds__(64) void l2_normalize_kernel(const T* x, int64_t ldx, float* out, int64_t ldo, int D) {
    const T* r = x + (int64_t)blockIdx.x * ldx;
    float* o = out + (int64_t)blockIdx.x * ldo;
    float s = 0.f;
    for (int k = threadIdx.x; k < D; k += 64) { const float v = (float)r[k]; s += v * v; }
    const float nrm = sqrtf(wave_sum(s));
    for (int k = threadIdx.x; k < D; k += 64) o[k] = (float)r[k] / nrm;
}

extern "C" int insv2v_l2_normalize(const void* x, int32_t fp32, int64_t ldx, float* out, int64_t ldo, int32_t n, int32_t D,
                                   insv2v_stream_t stream) {
    if (!one_device() || !x || !out || n <= 0 || D <= 0 || ldx < D || ldo < D) return INSV2V_EINVAL;
    if (fp32) hipLaunchKernelGGL(l2_normalize_kernel<float>, dim3(n), dim3(64), 0, as_stream(stream), (const float*)x, ldx, out, ldo, D);
    else hipLaunchKernelGGL(l2_normalize_kernel<half_t>, dim3(n), dim3(64), 0, as_stream(stream), (const half_t*)x, ldx, out, ldo, D);
    return launch_status();
}
