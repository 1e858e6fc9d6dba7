// Editing a region at full resolution: the box around a mask, the antialiased resampling of that box to the model's
// working size, and the paste of what the edit changed back into the full-resolution frames.  include/insv2v_hip.h states the
// definition, tests/region_ref.py restates it in float64.  Section 27 adds the same two operations with one real-valued box per frame
// (insv2v_region_resample_track, insv2v_region_paste_track; tests/region_track_ref.py): the kernels below share the device routine.
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

// One axis of a resampling.  The source has n_in samples (a box's, a cover's or the working image's), the destination n_out.  The box is
// real-valued (section 27): it starts ``off`` samples inside the cover and is ``ext`` samples long.  AXIS_DOWN (box -> working size):
// scale = ext / n_out, c = off + scale (i + 0.5).  AXIS_UP (working size -> cover): scale = n_in / ext, c = scale ((i + 0.5) - off).
// AXIS_INT is an integer box, off = 0.0 and ext = (double)n_in: AXIS_DOWN's numbers - the sum with 0.0 is exact - written as section 26
// wrote them, c = scale (i + 0.5), so that its kernels compile to the arithmetic they had and keep their bits.
enum { AXIS_INT = 0, AXIS_DOWN = 1, AXIS_UP = 2 };
struct Axis {
    int n_in, n_out;
    double off, ext;
    int form;
};
__device__ __forceinline__ Axis axis_int(int n_in, int n_out) { return Axis{n_in, n_out, 0.0, (double)n_in, AXIS_INT}; }

// the taps of destination index i of an axis: range in double (interpolate's own expressions), weights in fp32, normalised by their
// sum in tap order
__device__ __forceinline__ void axis_taps(int kind, const Axis& a, int i, float* w, int* first, int* count) {
    const int n_in = a.n_in;
    const double scale = a.form == AXIS_UP ? (double)n_in / a.ext : a.ext / (double)a.n_out, s = scale > 1.0 ? scale : 1.0;
    double c;
    if (a.form == AXIS_INT) {
        c = scale * ((double)i + 0.5);
    } else {   // product and sum rounded one by one: a contraction into an fma would round c differently from the definition
#pragma clang fp contract(off)
        const double at = (double)i + 0.5;
        c = a.form == AXIS_UP ? scale * (at - a.off) : a.off + scale * at;
    }
    const double sup = (kind == INSV2V_REGION_BILINEAR ? 1.0 : 2.0) * s;
    int lo = (int)(c - sup + 0.5), hi = (int)(c + sup + 0.5);
    lo = lo < 0 ? 0 : lo;
    hi = hi > n_in ? n_in : hi;
    int n = hi - lo;
    n = n > MAX_TAPS ? MAX_TAPS : n;   // (never beyond the ratio limit the entries enforce; an index into LDS all the same)
    if (a.form != AXIS_INT) n = n < 0 ? 0 : n;   // (a real-valued box never gives an empty range either; an index into LDS all the same)
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

// The tile (tile_x, tile_y) of a destination of ax.n_out x ay.n_out samples resampled from a source of ax.n_in x ay.n_in samples that
// ``load(y, x)`` reads: r[k] = the value of destination row tile_y * TILE_H + wave + k * WAVES, column tile_x * TILE_W + lane (0 outside the
// destination).  All 256 threads of the workgroup call it; it ends with a barrier, so it may be called again.
template <int ROWS, class Load>
__device__ __forceinline__ void resample_tile(Smem<ROWS>& sm, const Load& load, int kind, const Axis& ax, const Axis& ay, int tile_x, int tile_y,
                                              float r[PER_THREAD]) {
    const int out_w = ax.n_out, out_h = ay.n_out;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ox = tile_x * TILE_W + lane;
    if (tid < TILE_W) {
        if (ox < out_w) axis_taps(kind, ax, ox, sm.wx[tid], &sm.xmin[tid], &sm.xn[tid]);
        else sm.xmin[tid] = 0, sm.xn[tid] = 0;
    } else if (tid < TILE_W + TILE_H) {
        const int k = tid - TILE_W, oy = tile_y * TILE_H + k;
        if (oy < out_h) axis_taps(kind, ay, oy, sm.wy[k], &sm.ymin[k], &sm.yn[k]);
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
    resample_tile(sm, load, kind, axis_int(b.x1 - b.x0, w), axis_int(b.y1 - b.y0, h), blockIdx.x, blockIdx.y, r);
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
            resample_tile(sm, mload, INSV2V_REGION_BILINEAR, axis_int(w, bw), axis_int(h, bh), blockIdx.x, blockIdx.y, m);
        }
        const auto load = [&](int y, int x) { return edit[wp + (int64_t)y * w + x]; };
        resample_tile(sm, load, INSV2V_REGION_BICUBIC, axis_int(w, bw), axis_int(h, bh), blockIdx.x, blockIdx.y, r);
    } else {
        const auto load = [&](int y, int x) {
            const int64_t o = wp + (int64_t)y * w + x;
            return edit[o] - down[o];
        };
        resample_tile(sm, load, INSV2V_REGION_BICUBIC, axis_int(w, bw), axis_int(h, bh), blockIdx.x, blockIdx.y, r);
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

// ------------------------------------------------------------------------------------------------------------------ a box per frame
// Section 27: every frame has its own real-valued box.  The boxes of one launch (at most TRACK_CHUNK frames, 2 KiB) are a kernel
// argument: no device buffer, no copy, no synchronisation.  A frame's COVER is the integer box of the pixels its box touches; the
// resample reads the cover only, the paste writes the cover only.
constexpr int TRACK_CHUNK = 64;
struct TrackBoxes {
    double b[TRACK_CHUNK][4];
};
struct Cover {
    int X0, Y0, bw, bh;       // origin and size of the cover
    double x0, y0, x1, y1;    // the box
};
__device__ __forceinline__ Cover cover_of(const TrackBoxes& tb, int frame) {
    Cover c;
    c.x0 = tb.b[frame][0], c.y0 = tb.b[frame][1], c.x1 = tb.b[frame][2], c.y1 = tb.b[frame][3];
    c.X0 = (int)floor(c.x0), c.Y0 = (int)floor(c.y0);
    c.bw = (int)ceil(c.x1) - c.X0, c.bh = (int)ceil(c.y1) - c.Y0;
    return c;
}

template <int ROWS>
__global__ __launch_bounds__(256) void region_resample_track_kernel(const float* __restrict__ src, int64_t sn, int64_t sc, int64_t sh,
                                                                    float* __restrict__ dst, int C, int h, int w, TrackBoxes tb, int kind, int clamp,
                                                                    float lo, float hi) {
    __shared__ Smem<ROWS> sm;
    const int plane = blockIdx.z, n = plane / C, c = plane - n * C;
    const Cover cv = cover_of(tb, n);
    const float* p = src + (int64_t)n * sn + (int64_t)c * sc + (int64_t)cv.Y0 * sh + cv.X0;
    const auto load = [&](int y, int x) { return p[(int64_t)y * sh + x]; };
    const Axis ax{cv.bw, w, cv.x0 - (double)cv.X0, cv.x1 - cv.x0, AXIS_DOWN}, ay{cv.bh, h, cv.y0 - (double)cv.Y0, cv.y1 - cv.y0, AXIS_DOWN};
    float r[PER_THREAD];
    resample_tile(sm, load, kind, ax, ay, blockIdx.x, blockIdx.y, r);
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

// The paste into each frame's cover.  The grid is sized for the largest cover of the launch: a workgroup whose tile lies outside its
// own frame's cover leaves as a whole, before any barrier.
template <bool REPLACE, int ROWS>
__global__ __launch_bounds__(256) void region_paste_track_kernel(const float* __restrict__ edit, const float* __restrict__ down,
                                                                 const float* __restrict__ mask, int64_t mask_sn, float* __restrict__ out, int64_t on,
                                                                 int64_t oc, int64_t oh, int C, int H, int W, int h, int w, TrackBoxes tb, float blend) {
    __shared__ Smem<ROWS> sm;
    const int plane = blockIdx.z, n = plane / C, c = plane - n * C;
    const Cover cv = cover_of(tb, n);
    if ((int)blockIdx.x * TILE_W >= cv.bw || (int)blockIdx.y * TILE_H >= cv.bh) return;   // (uniform over the workgroup)
    const Axis ax{w, cv.bw, cv.x0 - (double)cv.X0, cv.x1 - cv.x0, AXIS_UP}, ay{h, cv.bh, cv.y0 - (double)cv.Y0, cv.y1 - cv.y0, AXIS_UP};
    const int64_t wp = (int64_t)plane * h * w;
    float r[PER_THREAD], m[PER_THREAD];
    if (REPLACE) {
        if (mask) {
            const float* mp = mask + (int64_t)n * mask_sn;
            const auto mload = [&](int y, int x) { return mp[(int64_t)y * w + x]; };
            resample_tile(sm, mload, INSV2V_REGION_BILINEAR, ax, ay, blockIdx.x, blockIdx.y, m);
        }
        const auto load = [&](int y, int x) { return edit[wp + (int64_t)y * w + x]; };
        resample_tile(sm, load, INSV2V_REGION_BICUBIC, ax, ay, blockIdx.x, blockIdx.y, r);
    } else {
        const auto load = [&](int y, int x) {
            const int64_t o = wp + (int64_t)y * w + x;
            return edit[o] - down[o];
        };
        resample_tile(sm, load, INSV2V_REGION_BICUBIC, ax, ay, blockIdx.x, blockIdx.y, r);
    }
    const int bx = blockIdx.x * TILE_W + (threadIdx.x & 63);
    if (bx >= cv.bw) return;
    // The signed distance from the pixel's centre to the nearest box edge that is not a frame border (exact in double: coordinates below
    // 2^24 with a fraction of a few bits), negative for a cover pixel whose centre lies outside the box.  ``in``: centre inside the
    // half-open box, which is what blend == 0 asks.
    const double big = 1e300, cx = (double)(cv.X0 + bx) + 0.5;
    const bool left = cv.x0 != 0.0, right = cv.x1 != (double)W, top = cv.y0 != 0.0, bottom = cv.y1 != (double)H;
    const double dx = fmin(left ? cx - cv.x0 : big, right ? cv.x1 - cx : big);
    const bool in_x = (!left || cx >= cv.x0) && (!right || cx < cv.x1);
    float* q = out + (int64_t)n * on + (int64_t)c * oc + (int64_t)cv.Y0 * oh + cv.X0 + bx;
#pragma unroll
    for (int k = 0; k < PER_THREAD; ++k) {
        const int by = blockIdx.y * TILE_H + (threadIdx.x >> 6) + k * WAVES;
        if (by >= cv.bh) continue;
        const double cy = (double)(cv.Y0 + by) + 0.5;
        const double d = fmin(dx, fmin(top ? cy - cv.y0 : big, bottom ? cv.y1 - cy : big));
        const bool in = in_x && (!top || cy >= cv.y0) && (!bottom || cy < cv.y1);
        float ramp = in ? 1.f : 0.f;
        if (blend > 0.f && d < big) ramp = fminf(1.f, fmaxf((float)d / blend, 0.f));
        const float s = q[(int64_t)by * oh];
        // a pixel under a ramp of 0 keeps the source; what was resampled for it is not used (half a pixel outside the box every tap of
        // the cubic can have the weight 0, and the normalised weights are then 0 / 0)
        // (the expressions of region_paste_kernel, statement for statement: the compiler then contracts the same products and sums,
        // which is what makes an integer box give that kernel's bits)
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
        if (ramp == 0.f) v = s;
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
bool sizes_ok(int32_t n, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w) {
    if (n < 1 || C < 1 || H < 1 || W < 1 || h < 1 || w < 1 || H > MAX_SIDE || W > MAX_SIDE || h > MAX_SIDE || w > MAX_SIDE) return false;
    if ((int64_t)n * C > 65535) return false;                          // planes ride on grid.z
    if (h > (int64_t)TILE_H * 65535) return false;                     // tile rows of either destination ride on grid.y
    return (int64_t)n * C <= MAX_ELEMS / ((int64_t)h * w);
}
bool geometry_ok(int32_t n, int32_t C, int32_t H, int32_t W, int32_t h, int32_t w, int32_t x0, int32_t y0, int32_t x1, int32_t y1) {
    if (!sizes_ok(n, C, H, W, h, w)) return false;
    if (x0 < 0 || y0 < 0 || x1 > W || y1 > H || x1 <= x0 || y1 <= y0) return false;
    const int64_t bw = x1 - x0, bh = y1 - y0;
    if (bw > (int64_t)MAX_RATIO * w || w > MAX_RATIO * bw || bh > (int64_t)MAX_RATIO * h || h > MAX_RATIO * bh) return false;
    return bh <= (int64_t)TILE_H * 65535;
}
// What the track entries need to know of their n boxes: every one finite, non-empty, inside the frame and within the ratio limit along
// both axes; the largest cover (the paste's grid) and the largest vertical ratios (the staging)
struct TrackInfo {
    int64_t cover_w, cover_h;
    double down_y, up_y;      // max over the frames of box height / h and of h / box height
};
bool track_ok(const double* boxes, int32_t n, int32_t H, int32_t W, int32_t h, int32_t w, TrackInfo* info) {
    if (!boxes) return false;
    *info = TrackInfo{0, 0, 0.0, 0.0};
    for (int32_t i = 0; i < n; ++i) {
        const double x0 = boxes[4 * i], y0 = boxes[4 * i + 1], x1 = boxes[4 * i + 2], y1 = boxes[4 * i + 3];
        if (!isfinite(x0) || !isfinite(y0) || !isfinite(x1) || !isfinite(y1)) return false;
        if (x0 < 0.0 || y0 < 0.0 || x1 > (double)W || y1 > (double)H || !(x1 > x0) || !(y1 > y0)) return false;
        const double ew = x1 - x0, eh = y1 - y0;
        if (!(ew > 0.0) || !(eh > 0.0)) return false;
        if (ew > (double)MAX_RATIO * w || w > (double)MAX_RATIO * ew || eh > (double)MAX_RATIO * h || h > (double)MAX_RATIO * eh) return false;
        const int64_t cw = (int64_t)ceil(x1) - (int64_t)floor(x0), ch = (int64_t)ceil(y1) - (int64_t)floor(y0);
        info->cover_w = cw > info->cover_w ? cw : info->cover_w, info->cover_h = ch > info->cover_h ? ch : info->cover_h;
        info->down_y = eh / h > info->down_y ? eh / h : info->down_y, info->up_y = h / eh > info->up_y ? h / eh : info->up_y;
    }
    return info->cover_h <= (int64_t)TILE_H * 65535;
}
TrackBoxes chunk_of(const double* boxes, int32_t first, int32_t count) {
    TrackBoxes tb;
    for (int i = 0; i < TRACK_CHUNK; ++i)
        for (int k = 0; k < 4; ++k) tb.b[i][k] = i < count ? boxes[4 * (int64_t)(first + i) + k] : 0.0;
    return tb;
}
// the smallest staging that holds the source rows under a tile: (TILE_H - 1) scale + 1 row starts apart, 2 support s + 1 taps each
// (a real-valued box changes nothing here: the first and the last row's centres are still (TILE_H - 1) scale apart, each range is
// int(c + support s + 0.5) - int(c - support s + 0.5) <= 2 support s + 1 long, at most 33 <= MAX_TAPS at the ratio limit)
int staging_rows(double scale) {
    const double s = scale > 1.0 ? scale : 1.0;
    const int need = (int)((TILE_H - 1) * scale) + 2 + (int)(4.0 * s) + 1;
    return need <= ROWS_UP ? ROWS_UP : need <= ROWS_MID ? ROWS_MID : MAX_ROWS;
}
int staging_rows(int64_t in_h, int64_t out_h) { return staging_rows((double)in_h / (double)out_h); }
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

// ------------------------------------------------------------------------------------------------------------------ a box per frame
extern "C" int insv2v_region_resample_track(const insv2v_region_resample_track_desc* d, insv2v_stream_t stream) {
    if (!d || !d->src || !d->dst) return INSV2V_EINVAL;
    if (!sizes_ok(d->n, d->C, d->H, d->W, d->h, d->w)) return INSV2V_EINVAL;
    TrackInfo info;
    if (!track_ok(d->boxes, d->n, d->H, d->W, d->h, d->w, &info)) return INSV2V_EINVAL;
    if (d->filter != INSV2V_REGION_BICUBIC && d->filter != INSV2V_REGION_BILINEAR) return INSV2V_EINVAL;
    if (d->clamp != 0 && d->clamp != 1) return INSV2V_EINVAL;
    if (d->clamp && !(d->clamp_lo <= d->clamp_hi)) return INSV2V_EINVAL;
    if (!view_ok(d->src, d->src_stride_n, d->src_stride_c, d->src_stride_h, d->n, d->C, d->H, d->W)) return INSV2V_EINVAL;
    const Span in = span_of(d->src, d->src_stride_n, d->src_stride_c, d->src_stride_h, d->n, d->C, d->H, d->W);
    const Span out{(uintptr_t)d->dst, (uintptr_t)((int64_t)d->n * d->C * d->h * d->w * 4)};
    if (overlap(in, out)) return INSV2V_EINVAL;
    const int rows = staging_rows(info.down_y);
    auto kern = rows == ROWS_UP ? region_resample_track_kernel<ROWS_UP> : rows == ROWS_MID ? region_resample_track_kernel<ROWS_MID> : region_resample_track_kernel<MAX_ROWS>;
    for (int32_t first = 0; first < d->n; first += TRACK_CHUNK) {
        const int32_t count = d->n - first < TRACK_CHUNK ? d->n - first : TRACK_CHUNK;
        hipLaunchKernelGGL(kern, tiles(d->w, d->h, (int64_t)count * d->C), dim3(256), 0, as_stream(stream), d->src + (int64_t)first * d->src_stride_n,
                           d->src_stride_n, d->src_stride_c, d->src_stride_h, d->dst + (int64_t)first * d->C * d->h * d->w, (int)d->C, (int)d->h,
                           (int)d->w, chunk_of(d->boxes, first, count), (int)d->filter, (int)d->clamp, d->clamp_lo, d->clamp_hi);
        const int rc = launch_status();
        if (rc) return rc;
    }
    return 0;
}

extern "C" int insv2v_region_paste_track(const insv2v_region_paste_track_desc* d, insv2v_stream_t stream) {
    if (!d || !d->edit || !d->out) return INSV2V_EINVAL;
    if (d->mode != INSV2V_REGION_RESIDUAL && d->mode != INSV2V_REGION_REPLACE) return INSV2V_EINVAL;
    const bool replace = d->mode == INSV2V_REGION_REPLACE;
    if (!replace && !d->down) return INSV2V_EINVAL;
    if (!sizes_ok(d->n, d->C, d->H, d->W, d->h, d->w)) return INSV2V_EINVAL;
    TrackInfo info;
    if (!track_ok(d->boxes, d->n, d->H, d->W, d->h, d->w, &info)) return INSV2V_EINVAL;
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
    const int rows = staging_rows(info.up_y);
    auto kern = replace ? (rows == ROWS_UP ? region_paste_track_kernel<true, ROWS_UP> : rows == ROWS_MID ? region_paste_track_kernel<true, ROWS_MID> : region_paste_track_kernel<true, MAX_ROWS>)
                        : (rows == ROWS_UP ? region_paste_track_kernel<false, ROWS_UP> : rows == ROWS_MID ? region_paste_track_kernel<false, ROWS_MID> : region_paste_track_kernel<false, MAX_ROWS>);
    for (int32_t first = 0; first < d->n; first += TRACK_CHUNK) {
        const int32_t count = d->n - first < TRACK_CHUNK ? d->n - first : TRACK_CHUNK;
        const int64_t wo = (int64_t)first * d->C * hw;
        hipLaunchKernelGGL(kern, tiles(info.cover_w, info.cover_h, (int64_t)count * d->C), dim3(256), 0, as_stream(stream), d->edit + wo,
                           replace ? (const float*)nullptr : d->down + wo, masked ? d->mask + (int64_t)first * d->mask_stride_n : (const float*)nullptr,
                           d->mask_stride_n, d->out + (int64_t)first * d->out_stride_n, d->out_stride_n, d->out_stride_c, d->out_stride_h, (int)d->C,
                           (int)d->H, (int)d->W, (int)d->h, (int)d->w, chunk_of(d->boxes, first, count), d->blend);
        const int rc = launch_status();
        if (rc) return rc;
    }
    return 0;
}
