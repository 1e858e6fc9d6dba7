// Scoring an edit in pixel space: the flow warp error of a video and the per-frame squared error / SSIM between
// two videos.  include/insv2v_hip.h states both definitions, tests/pixel_score_ref.py restates them in float64.  Both entries reduce in
// two stages with a fixed order - per-workgroup partial sums in the caller's workspace, then a finalize launch that adds them in index
// order in fp64 - so two calls give the same bits: no read-modify-write on global memory anywhere.
#include "common.h"
#include "flow_sample.h"
#include <math.h>

namespace {

struct View {   // insv2v_frames_view by value
    const void* p;
    int64_t st, sc, sh;
    float scale, shift;
};
// v = clamp(x * scale + shift, 0, 1) as the value is read (a NaN stays a NaN: it must show in the result, not be clamped away)
template <bool F32> __device__ __forceinline__ float rd(const View& v, int64_t off) {
    const float x = F32 ? ((const float*)v.p)[off] : (float)((const half_t*)v.p)[off];
    const float a = x * v.scale + v.shift;
    return a != a ? a : fminf(fmaxf(a, 0.f), 1.f);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// The NV sums of a 256-thread workgroup -> out[0 .. NV): a butterfly inside each wave, then the four waves in order.
template <int NV> __device__ __forceinline__ void block_sums(double (&v)[NV], double* sm /* [4 * NV] */, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double s = wave_sum_d(v[i]);
        if (lane == 0) sm[wave * NV + i] = s;
    }
    __syncthreads();
    if (threadIdx.x < NV) out[threadIdx.x] = ((sm[threadIdx.x] + sm[NV + threadIdx.x]) + sm[2 * NV + threadIdx.x]) + sm[3 * NV + threadIdx.x];
}
// sums[g][k] = the parts[g][0 .. n)[k] added in index order; one workgroup of 64 per g, lane k.
template <int NV> __global__ __launch_bounds__(64) void finalize_kernel(const double* __restrict__ parts, double* __restrict__ sums, int n) {
    if (threadIdx.x >= NV) return;
    const double* p = parts + (int64_t)blockIdx.x * n * NV + threadIdx.x;
    double s = 0.0;
#pragma unroll 8
    for (int i = 0; i < n; ++i) s += p[(int64_t)i * NV];
    sums[(int64_t)blockIdx.x * NV + threadIdx.x] = s;
}

// ------------------------------------------------------------------------------------------------------------------ warp error
constexpr int WE_PER = 8;                 // pixels per thread, 256 apart: consecutive threads walk a row
constexpr int WE_BLOCK = 256 * WE_PER;    // pixels per workgroup

template <bool F32>
__global__ __launch_bounds__(256) void warp_error_kernel(View a, const float* __restrict__ fwd, const float* __restrict__ bwd,
                                                         const float* __restrict__ w, double* __restrict__ parts,
                                                         float* __restrict__ err_map, float* __restrict__ valid_map, int H, int W,
                                                         float alpha, float beta) {
    __shared__ double sm[4 * 3];
    const int t = blockIdx.y;
    const int64_t plane = (int64_t)H * W;
    const float* b = fwd + (int64_t)t * 2 * plane;
    const float* c = bwd ? bwd + (int64_t)t * 2 * plane : nullptr;
    const int64_t f0 = (int64_t)t * a.st, f1 = f0 + a.st;
    double acc[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < WE_PER; ++k) {
        const int64_t r = (int64_t)blockIdx.x * WE_BLOCK + k * 256 + threadIdx.x;
        if (r >= plane) break;
        const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
        const float bx = b[r], by = b[plane + r];
        const float px = (float)x + bx, py = (float)y + by;
        const MtTaps tp = mt_taps(px, py, H, W);
        bool valid = mt_inb(px, py, H, W);
        if (c) valid = valid && mt_consistent(bx, by, mt_sample(tp, c), mt_sample(tp, c + plane), alpha, beta);
        float err = 0.f;
        if (valid) {
            float s = 0.f;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int64_t o1 = f1 + ch * a.sc;
                const float g = mt_lerp(tp, rd<F32>(a, o1 + tp.y0 * a.sh + tp.x0), rd<F32>(a, o1 + tp.y0 * a.sh + tp.x1),
                                        rd<F32>(a, o1 + tp.y1 * a.sh + tp.x0), rd<F32>(a, o1 + tp.y1 * a.sh + tp.x1));
                const float d = rd<F32>(a, f0 + ch * a.sc + y * a.sh + x) - g;
                s += d * d;
            }
            err = s / 3.f;
            const double wt = w ? (double)w[(int64_t)t * plane + r] : 1.0;
            acc[0] += wt * (double)err, acc[1] += wt, acc[2] += 1.0;
        }
        if (err_map) err_map[(int64_t)t * plane + r] = err;
        if (valid_map) valid_map[(int64_t)t * plane + r] = valid ? 1.f : 0.f;
    }
    block_sums<3>(acc, sm, parts + ((int64_t)t * gridDim.x + blockIdx.x) * 3);
}

// ------------------------------------------------------------------------------------------------------------------ fidelity
// A workgroup owns a tile of FT_H x FT_W SSIM centres and reads the (FT_H + 10) x (FT_W + 10) pixels under their windows once per
// channel into LDS (x - 1/2 and y - 1/2), runs the 11-tap row pass into five moment planes (a, b, a^2, b^2, ab) of (FT_H + 10) x FT_W
// and the column pass from those.  Consecutive lanes walk a row in every global read and in both passes, so the loads are coalesced
// and the LDS accesses hit consecutive banks.  2 * 26 * 74 + 5 * 26 * 64 floats = 48.7 KB of LDS: three workgroups per CU.
// The squared error is over ALL pixels, so each pixel is owned by exactly one tile: the pixels under its centres, and for a tile at a
// frame edge also the 5-pixel margin there.
constexpr int FT_H = 16, FT_W = 64, FT_R = 5;
constexpr int FR_H = FT_H + 2 * FT_R, FR_W = FT_W + 2 * FT_R;
constexpr int FR_N = FR_H * FR_W, FR_PER = (FR_N + 255) / 256;     // pixels of the region, and per thread
constexpr int FC_PER = FT_H * FT_W / 256;                            // centres per thread
constexpr int FM_N = FR_H * FT_W, FM_PER = (FM_N + 255) / 256;     // row-pass outputs, and per thread
struct Gauss { float g[11]; };
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;

template <bool XF32, bool YF32>
__global__ __launch_bounds__(256) void fidelity_kernel(View vx, View vy, const float* __restrict__ w, double* __restrict__ parts, int H,
                                                       int W, Gauss gw) {
    __shared__ float sa[FR_N], sb[FR_N];
    __shared__ float mom[5][FM_N];
    __shared__ double sm[4 * INSV2V_FIDELITY_K];
    const int t = blockIdx.z, tid = threadIdx.x;
    const int cy0 = blockIdx.y * FT_H, cx0 = blockIdx.x * FT_W;     // the region's first pixel = the tile's first centre - 5
    const int nCy = H - 2 * FT_R, nCx = W - 2 * FT_R;               // centres of the frame
    const bool lastx = blockIdx.x == gridDim.x - 1, lasty = blockIdx.y == gridDim.y - 1;
    // the pixels this tile owns, in region coordinates
    const int ox0 = blockIdx.x == 0 ? 0 : FT_R, ox1 = lastx ? W - cx0 : FT_W + FT_R;
    const int oy0 = blockIdx.y == 0 ? 0 : FT_R, oy1 = lasty ? H - cy0 : FT_H + FT_R;
    const int64_t plane = (int64_t)H * W;
    float dd[FR_PER], ss[FC_PER];
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) dd[k] = 0.f;
#pragma unroll
    for (int k = 0; k < FC_PER; ++k) ss[k] = 0.f;
    for (int ch = 0; ch < 3; ++ch) {
        const int64_t bx = (int64_t)t * vx.st + ch * vx.sc, by = (int64_t)t * vy.st + ch * vy.sc;
#pragma unroll
        for (int k = 0; k < FR_PER; ++k) {
            const int i = k * 256 + tid;
            if (i < FR_N) {
                const int ry = i / FR_W, rx = i - ry * FR_W;
                const int gy = cy0 + ry, gx = cx0 + rx;
                float a = 0.f, b = 0.f;
                if (gy < H && gx < W) {
                    const float xv = rd<XF32>(vx, bx + gy * vx.sh + gx), yv = rd<YF32>(vy, by + gy * vy.sh + gx);
                    const float d = xv - yv;
                    dd[k] += d * d;
                    a = xv - 0.5f, b = yv - 0.5f;
                }
                sa[i] = a, sb[i] = b;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FM_PER; ++k) {
            const int i = k * 256 + tid;
            if (i < FM_N) {
                const int ry = i / FT_W, cx = i - ry * FT_W;
                const float* pa = sa + ry * FR_W + cx;
                const float* pb = sb + ry * FR_W + cx;
                float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
                for (int j = 0; j < 11; ++j) {
                    const float a = pa[j], b = pb[j], g = gw.g[j];
                    m0 += g * a, m1 += g * b, m2 += g * (a * a), m3 += g * (b * b), m4 += g * (a * b);
                }
                mom[0][i] = m0, mom[1][i] = m1, mom[2][i] = m2, mom[3][i] = m3, mom[4][i] = m4;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < FC_PER; ++k) {
            const int i = k * 256 + tid;
            const int ty = i / FT_W, tx = i - ty * FT_W;
            if (cy0 + ty < nCy && cx0 + tx < nCx) {
                float m[5];
#pragma unroll
                for (int q = 0; q < 5; ++q) {
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < 11; ++j) s += gw.g[j] * mom[q][(ty + j) * FT_W + tx];
                    m[q] = s;
                }
                const float mx = m[0] + 0.5f, my = m[1] + 0.5f;
                const float sx2 = m[2] - m[0] * m[0], sy2 = m[3] - m[1] * m[1], sxy = m[4] - m[0] * m[1];
                const float num = (2.f * mx * my + SSIM_C1) * (2.f * sxy + SSIM_C2);
                const float den = (mx * mx + my * my + SSIM_C1) * (sx2 + sy2 + SSIM_C2);
                ss[k] += num / den;
            }
        }
        __syncthreads();   // the next channel overwrites sa / sb / mom
    }
    double acc[INSV2V_FIDELITY_K];
#pragma unroll
    for (int q = 0; q < INSV2V_FIDELITY_K; ++q) acc[q] = 0.0;
#pragma unroll
    for (int k = 0; k < FR_PER; ++k) {
        const int i = k * 256 + tid;
        const int ry = i / FR_W, rx = i - ry * FR_W;
        if (i < FR_N && ry >= oy0 && ry < oy1 && rx >= ox0 && rx < ox1) {   // (oy1 / ox1 keep the pixel inside the frame)
            const double se = (double)(dd[k] / 3.f);
            const double wt = w ? (double)w[(int64_t)t * plane + (int64_t)(cy0 + ry) * W + (cx0 + rx)] : 1.0;
            acc[0] += se, acc[1] += wt * se, acc[2] += (1.0 - wt) * se, acc[3] += wt, acc[4] += 1.0 - wt;
        }
    }
#pragma unroll
    for (int k = 0; k < FC_PER; ++k) {
        const int i = k * 256 + tid;
        const int ty = i / FT_W, tx = i - ty * FT_W;
        if (cy0 + ty < nCy && cx0 + tx < nCx) {
            const double s = (double)(ss[k] / 3.f);
            const double wc = w ? (double)w[(int64_t)t * plane + (int64_t)(cy0 + ty + FT_R) * W + (cx0 + tx + FT_R)] : 1.0;
            acc[5] += s, acc[6] += wc * s, acc[7] += (1.0 - wc) * s, acc[8] += wc, acc[9] += 1.0 - wc;
        }
    }
    const int64_t tile = ((int64_t)t * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    block_sums<INSV2V_FIDELITY_K>(acc, sm, parts + tile * INSV2V_FIDELITY_K);
}

// ------------------------------------------------------------------------------------------------------------------ host side
struct Span {
    uintptr_t lo, n;
};
Span span_of(const void* p, int64_t bytes) { return Span{(uintptr_t)p, p ? (uintptr_t)bytes : 0}; }
bool overlap(const Span& a, const Span& b) { return a.n && b.n && a.lo < b.lo + b.n && b.lo < a.lo + a.n; }
bool any_overlap(const Span* out, int no, const Span* in, int ni) {
    for (int o = 0; o < no; ++o) {
        for (int k = 0; k < ni; ++k)
            if (overlap(out[o], in[k])) return true;
        for (int p = 0; p < o; ++p)
            if (overlap(out[o], out[p])) return true;
    }
    return false;
}
constexpr int64_t MAX_SIDE = 1 << 24;             // pixel coordinates are exact in fp32
constexpr int64_t MAX_ELEMS = (int64_t)1 << 40;   // of any operand: no offset or byte count overflows int64
bool sizes_ok(int32_t T, int32_t H, int32_t W, int minT, int minSide) {
    if (T < minT || H < minSide || W < minSide || H > MAX_SIDE || W > MAX_SIDE) return false;
    return (int64_t)H * W <= MAX_ELEMS / 8 / T;
}
bool view_ok(const insv2v_frames_view& v, int32_t T, int32_t H, int32_t W) {
    if (!v.p || v.stride_t < 0 || v.stride_c < 0 || v.stride_h < W) return false;
    if (v.stride_t > MAX_ELEMS / T || v.stride_c > MAX_ELEMS / 3 || v.stride_h > MAX_ELEMS / H) return false;
    return isfinite(v.scale) && isfinite(v.shift);
}
Span view_span(const insv2v_frames_view& v, int32_t T, int32_t H, int32_t W) {
    const int64_t elems = (int64_t)(T - 1) * v.stride_t + 2 * v.stride_c + (int64_t)(H - 1) * v.stride_h + W;
    return span_of(v.p, elems * (v.fp32 ? 4 : 2));
}
View as_view(const insv2v_frames_view& v) { return View{v.p, v.stride_t, v.stride_c, v.stride_h, v.scale, v.shift}; }
int64_t we_blocks(int32_t H, int32_t W) { return ((int64_t)H * W + WE_BLOCK - 1) / WE_BLOCK; }
int64_t ft_tiles_x(int32_t W) { return (W - 2 * FT_R + FT_W - 1) / FT_W; }
int64_t ft_tiles_y(int32_t H) { return (H - 2 * FT_R + FT_H - 1) / FT_H; }

}   // namespace

extern "C" int64_t insv2v_warp_error_workspace_bytes(int32_t T, int32_t H, int32_t W) {
    if (!sizes_ok(T, H, W, 2, 2) || T - 1 > 65535 || we_blocks(H, W) > 0x7fffffffll) return INSV2V_EINVAL;
    return (int64_t)(T - 1) * we_blocks(H, W) * 3 * (int64_t)sizeof(double);
}

extern "C" int insv2v_warp_error(const insv2v_warp_error_desc* d, insv2v_stream_t stream) {
    if (!d || !d->fwd || !d->sums || !d->workspace) return INSV2V_EINVAL;
    const int64_t need = insv2v_warp_error_workspace_bytes(d->T, d->H, d->W);
    if (need <= 0 || d->workspace_bytes < need || !view_ok(d->a, d->T, d->H, d->W)) return INSV2V_EINVAL;
    if (!(d->alpha >= 0.f) || !(d->beta >= 0.f) || !isfinite(d->alpha) || !isfinite(d->beta)) return INSV2V_EINVAL;
    if ((uintptr_t)d->workspace % 8 || (uintptr_t)d->sums % 8) return INSV2V_EINVAL;
    const int64_t plane = (int64_t)d->H * d->W, P = d->T - 1;
    const Span in[4] = {view_span(d->a, d->T, d->H, d->W), span_of(d->fwd, P * 2 * plane * 4), span_of(d->bwd, P * 2 * plane * 4),
                        span_of(d->w, (int64_t)d->T * plane * 4)};
    const Span out[4] = {span_of(d->sums, P * 3 * 8), span_of(d->err_map, P * plane * 4), span_of(d->valid_map, P * plane * 4),
                         span_of(d->workspace, need)};
    if (any_overlap(out, 4, in, 4)) return INSV2V_EINVAL;
    const int nblk = (int)we_blocks(d->H, d->W);
    const dim3 grid((unsigned)nblk, (unsigned)P);
    double* parts = (double*)d->workspace;
    auto kern = d->a.fp32 ? warp_error_kernel<true> : warp_error_kernel<false>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, as_stream(stream), as_view(d->a), d->fwd, d->bwd, d->w, parts, d->err_map, d->valid_map,
                       (int)d->H, (int)d->W, d->alpha, d->beta);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(finalize_kernel<3>, dim3((unsigned)P), dim3(64), 0, as_stream(stream), (const double*)parts, d->sums, nblk);
    return launch_status();
}

extern "C" int insv2v_frame_fidelity_tile(int32_t* rows, int32_t* cols) {
    if (rows) *rows = FT_H;
    if (cols) *cols = FT_W;
    return 0;
}

extern "C" int64_t insv2v_frame_fidelity_workspace_bytes(int32_t T, int32_t H, int32_t W) {
    if (!sizes_ok(T, H, W, 1, 2 * FT_R + 1) || T > 65535 || ft_tiles_y(H) > 65535 || ft_tiles_x(W) > 0x7fffffffll) return INSV2V_EINVAL;
    return (int64_t)T * ft_tiles_y(H) * ft_tiles_x(W) * INSV2V_FIDELITY_K * (int64_t)sizeof(double);
}

extern "C" int insv2v_frame_fidelity(const insv2v_fidelity_desc* d, insv2v_stream_t stream) {
    if (!d || !d->sums || !d->workspace) return INSV2V_EINVAL;
    const int64_t need = insv2v_frame_fidelity_workspace_bytes(d->T, d->H, d->W);
    if (need <= 0 || d->workspace_bytes < need || !view_ok(d->x, d->T, d->H, d->W) || !view_ok(d->y, d->T, d->H, d->W)) return INSV2V_EINVAL;
    if ((uintptr_t)d->workspace % 8 || (uintptr_t)d->sums % 8) return INSV2V_EINVAL;
    const int64_t plane = (int64_t)d->H * d->W;
    const Span in[3] = {view_span(d->x, d->T, d->H, d->W), view_span(d->y, d->T, d->H, d->W), span_of(d->w, (int64_t)d->T * plane * 4)};
    const Span out[2] = {span_of(d->sums, (int64_t)d->T * INSV2V_FIDELITY_K * 8), span_of(d->workspace, need)};
    if (any_overlap(out, 2, in, 3)) return INSV2V_EINVAL;
    Gauss gw;
    double g[11], sum = 0.0;
    for (int k = 0; k < 11; ++k) sum += g[k] = exp(-(double)((k - 5) * (k - 5)) / (2.0 * 1.5 * 1.5));
    for (int k = 0; k < 11; ++k) gw.g[k] = (float)(g[k] / sum);
    const int tx = (int)ft_tiles_x(d->W), ty = (int)ft_tiles_y(d->H);
    const dim3 grid((unsigned)tx, (unsigned)ty, (unsigned)d->T);
    double* parts = (double*)d->workspace;
    auto kern = d->x.fp32 ? (d->y.fp32 ? fidelity_kernel<true, true> : fidelity_kernel<true, false>)
                          : (d->y.fp32 ? fidelity_kernel<false, true> : fidelity_kernel<false, false>);
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, as_stream(stream), as_view(d->x), as_view(d->y), d->w, parts, (int)d->H, (int)d->W, gw);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(finalize_kernel<INSV2V_FIDELITY_K>, dim3((unsigned)d->T), dim3(64), 0, as_stream(stream), (const double*)parts,
                       d->sums, tx * ty);
    return launch_status();
}
