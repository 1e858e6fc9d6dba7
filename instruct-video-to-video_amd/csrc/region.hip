// Editing a region at full resolution: the box around a mask, the antialiased resampling of that box to the model's
// working size, and the paste of what the edit changed back into the full-resolution frames.  include/insv2v_hip.h states the
// definition, tests/region_ref.py restates it in float64.
//
// One device routine serves the resample and the paste: a workgroup of 4 waves owns a TILE_H x TILE_W tile of the DESTINATION of one
// plane.  It evaluates the tile's tap tables once (centres and tap ranges in double, weights in fp32, normalised by their sum in tap
// order), runs the HORIZONTAL pass of the source rows the tile needs into LDS (a wave per row, a lane per destination column: the
// stores to LDS are conflict-free, the loads of neighbouring lanes overlap and are served by the vector L1) and then the VERTICAL pass
// from LDS (lanes walk a destination row: conflict-free reads, coalesced stores).  No intermediate image exists in HBM; that a source
// element is read from HBM only once per tile whose halo holds it is an ASSUMPTION about the L1, not a measurement - the kernels run at
// 0.2 - 0.4 of a copy's rate (profiles/region_gpu.txt).  Every destination element is a sum in tap order formed by one thread:
// no atomics, two calls give the same bits.  With equal sizes the weights are exactly 0, 1, 0, 0 and the box is copied bit for bit.
// The ratio limit of 8 per axis is what bounds the staging: MAX_ROWS rows of TILE_W fp32 values.
// Plain pointers with 64-bit element offsets (nothing has to fit a window).
#include "common.h"
#include <math.h>

namespace {

constexpr int TILE_W = 64, TILE_H = 16, WAVES = 4, PER_THREAD = TILE_H / WAVES;
constexpr int MAX_TAPS = 34;                                  // 2 * support * 8 + 1 = 33 for the cubic at the ratio limit
constexpr int TAP_LD = 37;                                    // MAX_TAPS rounded up to the unroll of 4, and odd: the lanes' rows of the x table fall into different banks
constexpr int MAX_ROWS = (TILE_H - 1) * 8 + 1 + MAX_TAPS;     // source rows under a tile at the ratio limit (155)
constexpr int MAX_RATIO = 8;
// The staging is sized by the vertical ratio (the launchers choose): up-sampling (the paste) needs 21 rows under a tile, a ratio up to
// 3 needs 60 - so 8 and 5 workgroups fit a CU's LDS instead of 3, and the loads of more waves hide one another's latency.
constexpr int ROWS_UP = 24, ROWS_MID = 64;

template <int ROWS>
struct Smem {
    float h[ROWS][TILE_W];              // the horizontal pass of the tile's source rows
    float wx[TILE_W][TAP_LD], wy[TILE_H][TAP_LD];
    int xmin[TILE_W], xn[TILE_W], ymin[TILE_H], yn[TILE_H];
};

__device__ __forceinline__ float filter_w(int kind, float t) {
    t = fabsf(t);
    if (kind == INSV2V_REGION_BILINEAR) return t < 1.f ? 1.f - t : 0.f;
    const float A = -0.5f;
    if (t < 1.f) return ((A + 2.f) * t - (A + 3.f)) * t * t + 1.f;
    if (t < 2.f) return (t - 1.f) * (t - 2.f) * (t - 2.f) * A;   // ((t - 5) t + 8) t - 4 factored: no cancellation among terms of size 16
    return 0.f;
}

// the taps of destination index i of an axis with n_in source and n_out destination samples: range in double (interpolate's own
// expressions), weights in fp32, normalised by their sum in tap order
__device__ __forceinline__ void axis_taps(int kind, int n_in, int n_out, int i, float* w, int* first, int* count) {
    const double scale = (double)n_in / (double)n_out, s = scale > 1.0 ? scale : 1.0;
    const double sup = (kind == INSV2V_REGION_BILINEAR ? 1.0 : 2.0) * s, c = scale * ((double)i + 0.5);
    int lo = (int)(c - sup + 0.5), hi = (int)(c + sup + 0.5);
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_in ? n_in : hi;
    int n = hi - lo;
    n = n > MAX_TAPS ? MAX_TAPS : n;   // (never beyond the ratio limit the entries enforce; an index into LDS all the same)
    float total = 0.f;
    for (int j = 0; j < n; ++j) {
        const float v = filter_w(kind, (float)(((double)(lo + j) - c + 0.5) / s));   // the argument rounded once
        w[j] = v;
        total += v;
    }
    for (int j = 0; j < n; ++j) w[j] = w[j] / total;
    for (int j = n; j < ((n + 3) & ~3); ++j) w[j] = 0.f;   // the passes run in steps of 4 taps: a padded tap adds exactly 0 x (one of its own taps)
    *first = lo;
    *count = n;
}

// The tile (tile_x, tile_y) of a destination of out_w x out_h samples resampled from a source of in_w x in_h samples that ``load(y, x)``
// reads: r[k] = the value of destination row tile_y * TILE_H + wave + k * WAVES, column tile_x * TILE_W + lane (0 outside the
// destination).  All 256 threads of the workgroup call it; it ends with a barrier, so it may be called again.
template <int ROWS, class Load>
__device__ __forceinline__ void resample_tile(Smem<ROWS>& sm, const Load& load, int kind, int in_w, int in_h, int out_w, int out_h, int tile_x,
                                              int tile_y, float r[PER_THREAD]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ox = tile_x * TILE_W + lane;
    if (tid < TILE_W) {
        if (ox < out_w) axis_taps(kind, in_w, out_w, ox, sm.wx[tid], &sm.xmin[tid], &sm.xn[tid]);
        else sm.xmin[tid] = 0, sm.xn[tid] = 0;
    } else if (tid < TILE_W + TILE_H) {
        const int k = tid - TILE_W, oy = tile_y * TILE_H + k;
        if (oy < out_h) axis_taps(kind, in_h, out_h, oy, sm.wy[k], &sm.ymin[k], &sm.yn[k]);
        else sm.ymin[k] = 0, sm.yn[k] = 0;
    }
    __syncthreads();
    const int rows_here = min(TILE_H, out_h - tile_y * TILE_H);
    const int y_lo = sm.ymin[0];
    int y_hi = sm.ymin[rows_here - 1] + sm.yn[rows_here - 1];   // the tap ranges move monotonically with the destination row
    y_hi = min(y_hi, y_lo + ROWS);
    // Two rows and four taps at a time: eight independent loads are in flight before the first is used.  Each sum is still formed in
    // tap order; a tap beyond the lane's count has weight 0 and re-reads the lane's last tap.
    const int x_first = sm.xmin[lane], x_count = sm.xn[lane], x_last = x_first + max(x_count - 1, 0);
    for (int y = y_lo + wave; y < y_hi; y += 2 * WAVES) {
        const int yb = min(y + WAVES, y_hi - 1);   // (the last pair of a wave may hold one row: it is then computed twice)
        float acc_a = 0.f, acc_b = 0.f;
        for (int j = 0; j < x_count; j += 4) {
            float va[4], vb[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int x = min(x_first + j + u, x_last);
                va[u] = load(y, x), vb[u] = load(yb, x);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float wt = sm.wx[lane][j + u];
                acc_a = fmaf(wt, va[u], acc_a), acc_b = fmaf(wt, vb[u], acc_b);
            }
        }
        sm.h[y - y_lo][lane] = acc_a;
        if (y + WAVES < y_hi) sm.h[yb - y_lo][lane] = acc_b;
    }
    __syncthreads();
    int first[PER_THREAD], count[PER_THREAD], longest = 0;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int row = wave + k * WAVES;
        const bool live = row < rows_here && ox < out_w;
        first[k] = live ? sm.ymin[row] - y_lo : 0;
        count[k] = live ? max(min(sm.yn[row], ROWS - first[k]), 0) : 0;
        longest = max(longest, count[k]);
        r[k] = 0.f;
    }
    for (int j = 0; j < longest; j += 4) {     // the thread's four destination rows side by side, four taps at a time
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int k = 0; k < PER_THREAD; ++k) {
                if (j + u < count[k]) r[k] = fmaf(sm.wy[wave + k * WAVES][j + u], sm.h[first[k] + j + u][lane], r[k]);
            }
        }
    }
    __syncthreads();
}

struct Box {
    int x0, y0, x1, y1;
};

template <int ROWS>
__global__ __launch_bounds__(256) void region_resample_kernel(const float* __restrict__ src, int64_t sn, int64_t sc, int64_t sh, float* __restrict__ dst,
                                                              int C, int h, int w, Box b, int kind, int clamp, float lo, float hi) {
    __shared__ Smem<ROWS> sm;
    const int plane = blockIdx.z, n = plane / C, c = plane - n * C;
    const float* p = src + (int64_t)n * sn + (int64_t)c * sc + (int64_t)b.y0 * sh + b.x0;
    const auto load = [&](int y, int x) { return p[(int64_t)y * sh + x]; };
    float r[PER_THREAD];
    resample_tile(sm, load, kind, b.x1 - b.x0, b.y1 - b.y0, w, h, blockIdx.x, blockIdx.y, r);
    const int ox = blockIdx.x * TILE_W + (threadIdx.x & 63);
    if (ox >= w) return;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int oy = blockIdx.y * TILE_H + (threadIdx.x >> 6) + k * WAVES;
        if (oy >= h) continue;
        float v = r[k];
        if (clamp) v = v != v ? v : fminf(fmaxf(v, lo), hi);
        dst[((int64_t)plane * h + oy) * w + ox] = v;
    }
}

// The paste: the working-resolution operand (edit - down, or edit) formed at load, resampled to the box and blended into out, whose
// box still holds the source - a thread reads its pixel before it writes it.
template <bool REPLACE, int ROWS>
__global__ __launch_bounds__(256) void region_paste_kernel(const float* __restrict__ edit, const float* __restrict__ down, const float* __restrict__ mask,
                                                           int64_t mask_sn, float* __restrict__ out, int64_t on, int64_t oc, int64_t oh, int C, int H, int W,
                                                           int h, int w, Box b, float blend) {
    __shared__ Smem<ROWS> sm;
    const int plane = blockIdx.z, n = plane / C, c = plane - n * C;
    const int bw = b.x1 - b.x0, bh = b.y1 - b.y0;
    const int64_t wp = (int64_t)plane * h * w;
    float r[PER_THREAD], m[PER_THREAD];
    if (REPLACE) {
        if (mask) {
            const float* mp = mask + (int64_t)n * mask_sn;
            const auto mload = [&](int y, int x) { return mp[(int64_t)y * w + x]; };
            resample_tile(sm, mload, INSV2V_REGION_BILINEAR, w, h, bw, bh, blockIdx.x, blockIdx.y, m);
        }
        const auto load = [&](int y, int x) { return edit[wp + (int64_t)y * w + x]; };
        resample_tile(sm, load, INSV2V_REGION_BICUBIC, w, h, bw, bh, blockIdx.x, blockIdx.y, r);
    } else {
        const auto load = [&](int y, int x) {
            const int64_t o = wp + (int64_t)y * w + x;
            return edit[o] - down[o];
        };
        resample_tile(sm, load, INSV2V_REGION_BICUBIC, w, h, bw, bh, blockIdx.x, blockIdx.y, r);
    }
    const int bx = blockIdx.x * TILE_W + (threadIdx.x & 63);
    if (bx >= bw) return;
    // the distance to the nearest box edge that is not also a frame border (the box lies inside a frame of at most 2^24 pixels a side)
    const int big = 1 << 30;
    const int dx = min(b.x0 > 0 ? bx : big, b.x1 < W ? bw - 1 - bx : big);
    float* q = out + (int64_t)n * on + (int64_t)c * oc + (int64_t)b.y0 * oh + b.x0 + bx;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int by = blockIdx.y * TILE_H + (threadIdx.x >> 6) + k * WAVES;
        if (by >= bh) continue;
        const int d = min(dx, min(b.y0 > 0 ? by : big, b.y1 < H ? bh - 1 - by : big));
        float ramp = 1.f;
        if (blend > 0.f && d < big) ramp = fminf(1.f, ((float)d + 0.5f) / blend);
        const float s = q[(int64_t)by * oh];
        float v;
        if (REPLACE) {
            float M = ramp;
            if (mask) M = ramp * fminf(fmaxf(m[k], 0.f), 1.f);
            const float add = M * (r[k] - s);
            v = add == 0.f ? s : s + add;   // nothing to add leaves the source's bits (also those of a -0)
        } else {
            const float add = ramp * r[k];
            v = add == 0.f ? s : s + add;
        }
        q[(int64_t)by * oh] = v != v ? v : fminf(fmaxf(v, -1.f), 1.f);
    }
}

// ------------------------------------------------------------------------------------------------------------------ the bounding box
constexpr int BBOX_PER_THREAD = 8;

__global__ void bbox_init_kernel(int32_t* boxes, int T, int H, int W) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i > T) return;
    boxes[4 * i + 0] = W, boxes[4 * i + 1] = H, boxes[4 * i + 2] = 0, boxes[4 * i + 3] = 0;
}

// min and max commute: whatever order the workgroups arrive in, the result is a function of the mask only
__global__ __launch_bounds__(256) void mask_bbox_kernel(const float* __restrict__ m, int64_t st, int64_t sh, int32_t* boxes, int T, int H, int W,
                                                        float threshold) {
    __shared__ int part[4][4];
    const int t = blockIdx.y;
    const int64_t plane = (int64_t)H * W;
    int x0 = W, y0 = H, x1 = 0, y1 = 0;
#pragma unroll
    for (int k = 0; k < BBOX_PER_THREAD; ++k) {
        const int64_t r = ((int64_t)blockIdx.x * BBOX_PER_THREAD + k) * 256 + threadIdx.x;
        if (r >= plane) break;
        const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
        if (m[(int64_t)t * st + (int64_t)y * sh + x] > threshold) {   // strict; a NaN is outside
            x0 = min(x0, x), y0 = min(y0, y), x1 = max(x1, x + 1), y1 = max(y1, y + 1);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        x0 = min(x0, __shfl_xor(x0, o, 64)), y0 = min(y0, __shfl_xor(y0, o, 64));
        x1 = max(x1, __shfl_xor(x1, o, 64)), y1 = max(y1, __shfl_xor(y1, o, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) part[wave][0] = x0, part[wave][1] = y0, part[wave][2] = x1, part[wave][3] = y1;
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int v = 1; v < 4; ++v) x0 = min(x0, part[v][0]), y0 = min(y0, part[v][1]), x1 = max(x1, part[v][2]), y1 = max(y1, part[v][3]);
    if (x1 == 0) return;   // nothing inside this workgroup's pixels
    for (int i = 0; i < 2; ++i) {
        int32_t* b = boxes + 4 * (i ? T : t);
        atomicMin(b + 0, x0), atomicMin(b + 1, y0), atomicMax(b + 2, x1), atomicMax(b + 3, y1);
    }
}

// ------------------------------------------------------------------------------------------------------------------ host side
constexpr int64_t MAX_SIDE = 1 << 24;
constexpr int64_t MAX_ELEMS = (int64_t)1 << 40;   // of any operand: no offset or byte count overflows int64

struct Span {
    uintptr_t lo, n;
};
bool overlap(const Span& a, const Span& b) { return a.n && b.n && a.lo < b.lo + b.n && b.lo < a.lo + a.n; }

bool view_ok(const void* p, int64_t sn, int64_t sc, int64_t sh, int64_t n, int64_t C, int64_t H, int64_t W) {
    if (!p || sn < 0 || sc < 0 || sh < W) return false;
    return sn <= MAX_ELEMS / n && sc <= MAX_ELEMS / C && sh <= MAX_ELEMS / H;
}
Span span_of(const void* p, int64_t sn, int64_t sc, int64_t sh, int64_t n, int64_t C, int64_t H, int64_t W) {
    return Span{(uintptr_t)p, (uintptr_t)(((n - 1) * sn + (C - 1) * sc + (H - 1) * sh + W) * 4)};
}
// a frame, a box inside it and a working size the kernels can run: positive sizes, a non-empty box, per-axis ratios inside [1/8, 8]
bool geometry_ok(int32_t n, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
    if (n < 1 || C < 1 || H < 1 || W < 1 || h < 1 || w < 1 || H > MAX_SIDE || W > MAX_SIDE || h > MAX_SIDE || w > MAX_SIDE) return false;
    if (x0 < 0 || y0 < 0 || x1 > W || y1 > H || x1 <= x0 || y1 <= y0) return false;
    const int64_t bw = x1 - x0, bh = y1 - y0;
    if (bw > (int64_t)MAX_RATIO * w || w > MAX_RATIO * bw || bh > (int64_t)MAX_RATIO * h || h > MAX_RATIO * bh) return false;
    if ((int64_t)n * C > 65535) return false;                          // planes ride on grid.z
    if (h > (int64_t)TILE_H * 65535 || bh > (int64_t)TILE_H * 65535) return false;   // tile rows of either destination ride on grid.y
    return (int64_t)n * C <= MAX_ELEMS / ((int64_t)h * w);
}
// the smallest staging that holds the source rows under a tile: (TILE_H - 1) scale + 1 row starts apart, 2 support s + 1 taps each
int staging_rows(int64_t in_h, int64_t out_h) {
    const double scale = (double)in_h / (double)out_h, s = scale > 1.0 ? scale : 1.0;
    const int need = (int)((TILE_H - 1) * scale) + 2 + (int)(4.0 * s) + 1;
    return need <= ROWS_UP ? ROWS_UP : need <= ROWS_MID ? ROWS_MID : MAX_ROWS;
}
dim3 tiles(int64_t out_w, int64_t out_h, int64_t planes) {
    return dim3((unsigned)((out_w + TILE_W - 1) / TILE_W), (unsigned)((out_h + TILE_H - 1) / TILE_H), (unsigned)planes);
}

}   // namespace

extern "C" int insv2v_mask_bbox(const float* mask, int64_t stride_t, int64_t stride_h, int32_t T, int32_t H, int32_t W, float threshold,
                                int32_t* boxes, insv2v_stream_t stream) {
    if (!mask || !boxes || T < 1 || H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE || T > 65534) return INSV2V_EINVAL;
    if (stride_t < 0 || stride_h < W || stride_t > MAX_ELEMS / T || stride_h > MAX_ELEMS / H || !isfinite(threshold)) return INSV2V_EINVAL;
    const int64_t per_block = 256 * BBOX_PER_THREAD, blocks = ((int64_t)H * W + per_block - 1) / per_block;
    if (blocks > 0x7fffffffll) return INSV2V_EINVAL;
    const Span in = span_of(mask, stride_t, 0, stride_h, T, 1, H, W), out{(uintptr_t)boxes, (uintptr_t)(T + 1) * 16};
    if (overlap(in, out)) return INSV2V_EINVAL;
    hipLaunchKernelGGL(bbox_init_kernel, dim3((unsigned)(T / 256 + 1)), dim3(256), 0, as_stream(stream), boxes, (int)T, (int)H, (int)W);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(mask_bbox_kernel, dim3((unsigned)blocks, (unsigned)T), dim3(256), 0, as_stream(stream), mask, stride_t, stride_h, boxes,
                       (int)T, (int)H, (int)W, threshold);
    return launch_status();
}

extern "C" int insv2v_region_resample(const insv2v_region_resample_desc* d, insv2v_stream_t stream) {
    if (!d || !d->src || !d->dst) return INSV2V_EINVAL;
    if (!geometry_ok(d->n, d->C, d->H, d->W, d->h, d->w, d->x0, d->y0, d->x1, d->y1)) return INSV2V_EINVAL;
    if (d->filter != INSV2V_REGION_BICUBIC && d->filter != INSV2V_REGION_BILINEAR) return INSV2V_EINVAL;
    if (d->clamp != 0 && d->clamp != 1) return INSV2V_EINVAL;
    if (d->clamp && !(d->clamp_lo <= d->clamp_hi)) return INSV2V_EINVAL;
    if (!view_ok(d->src, d->src_stride_n, d->src_stride_c, d->src_stride_h, d->n, d->C, d->H, d->W)) return INSV2V_EINVAL;
    const Span in = span_of(d->src, d->src_stride_n, d->src_stride_c, d->src_stride_h, d->n, d->C, d->H, d->W);
    const Span out{(uintptr_t)d->dst, (uintptr_t)((int64_t)d->n * d->C * d->h * d->w * 4)};
    if (overlap(in, out)) return INSV2V_EINVAL;
    const Box box{d->x0, d->y0, d->x1, d->y1};
    const int rows = staging_rows(d->y1 - d->y0, d->h);
    auto kern = rows == ROWS_UP ? region_resample_kernel<ROWS_UP> : rows == ROWS_MID ? region_resample_kernel<ROWS_MID> : region_resample_kernel<MAX_ROWS>;
    hipLaunchKernelGGL(kern, tiles(d->w, d->h, (int64_t)d->n * d->C), dim3(256), 0, as_stream(stream), d->src, d->src_stride_n,
                       d->src_stride_c, d->src_stride_h, d->dst, (int)d->C, (int)d->h, (int)d->w, box, (int)d->filter,
                       (int)d->clamp, d->clamp_lo, d->clamp_hi);
    return launch_status();
}

extern "C" int insv2v_region_paste(const insv2v_region_paste_desc* d, insv2v_stream_t stream) {
    if (!d || !d->edit || !d->out) return INSV2V_EINVAL;
    if (d->mode != INSV2V_REGION_RESIDUAL && d->mode != INSV2V_REGION_REPLACE) return INSV2V_EINVAL;
    const bool replace = d->mode == INSV2V_REGION_REPLACE;
    if (!replace && !d->down) return INSV2V_EINVAL;
    if (!geometry_ok(d->n, d->C, d->H, d->W, d->h, d->w, d->x0, d->y0, d->x1, d->y1)) return INSV2V_EINVAL;
    if (!isfinite(d->blend) || d->blend < 0.f) return INSV2V_EINVAL;
    if (!view_ok(d->out, d->out_stride_n, d->out_stride_c, d->out_stride_h, d->n, d->C, d->H, d->W)) return INSV2V_EINVAL;
    const int64_t hw = (int64_t)d->h * d->w;
    const bool masked = replace && d->mask;
    if (masked && (d->mask_stride_n < 0 || (d->mask_stride_n != 0 && d->mask_stride_n < hw) || d->mask_stride_n > MAX_ELEMS / d->n)) return INSV2V_EINVAL;
    const Span o = span_of(d->out, d->out_stride_n, d->out_stride_c, d->out_stride_h, d->n, d->C, d->H, d->W);
    const uintptr_t wbytes = (uintptr_t)((int64_t)d->n * d->C * hw * 4);
    const Span in[3] = {Span{(uintptr_t)d->edit, wbytes}, Span{(uintptr_t)d->down, replace ? 0 : wbytes},
                        Span{(uintptr_t)d->mask, masked ? (uintptr_t)(((int64_t)(d->n - 1) * d->mask_stride_n + hw) * 4) : 0}};
    for (int i = 0; i < 3; ++i)
        if (overlap(o, in[i])) return INSV2V_EINVAL;
    const int rows = staging_rows(d->h, d->y1 - d->y0);
    auto kern = replace ? (rows == ROWS_UP ? region_paste_kernel<true, ROWS_UP> : rows == ROWS_MID ? region_paste_kernel<true, ROWS_MID> : region_paste_kernel<true, MAX_ROWS>)
                        : (rows == ROWS_UP ? region_paste_kernel<false, ROWS_UP> : rows == ROWS_MID ? region_paste_kernel<false, ROWS_MID> : region_paste_kernel<false, MAX_ROWS>);
    const Box box{d->x0, d->y0, d->x1, d->y1};
    hipLaunchKernelGGL(kern, tiles(d->x1 - d->x0, d->y1 - d->y0, (int64_t)d->n * d->C), dim3(256), 0, as_stream(stream), d->edit, d->down,
                       masked ? d->mask : (const float*)nullptr, d->mask_stride_n, d->out, d->out_stride_n, d->out_stride_c, d->out_stride_h, (int)d->C,
                       (int)d->H, (int)d->W, (int)d->h, (int)d->w, box, d->blend);
    return launch_status();
}
