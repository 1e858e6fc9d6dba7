// Growing, shrinking and feathering a mask: an exact Euclidean distance transform inside a radius R <= 64, the
// two hard decisions on its integers, the ramp in fp32.  include/insv2v_hip.h states the definition, tests/mask_shape_ref.py restates it
// with integers and float64, mask_shape_plan.h turns (grow, feather) into R and the four integer thresholds.
// The squared distance separates: D2(x, y) = min over dx of dx^2 + v(x + dx, y)^2 with v the vertical distance to the nearest pixel of
// the set in a column.  A column pass writes v for both sets as ONE signed byte per pixel (a pixel is inside or outside, so one of the two
// distances is 0: +v_inside on outside pixels, -v_outside on inside pixels, each capped at R + 1 <= 65); a row pass stages a row segment
// and its R-wide halo in LDS as the two squares and takes the minimum over the window.  Consecutive lanes walk a row in every global
// access and every LDS access.  Each thread writes its own pixels with plain stores: no atomics, nothing depends on the launch order.
#include "common.h"
#include "mask_shape_plan.h"
#include <math.h>

namespace {

constexpr int MS_TILE = MASK_SHAPE_ROW_TILE;   // pixels per workgroup along a row, one per thread, in both passes
constexpr int MS_CH = 32;                      // rows of a column one thread of the column pass owns
constexpr int MS_MAXR = 2 * INSV2V_MASK_SHAPE_MAX;   // R <= g + f <= 64
static_assert(MS_TILE == 256, "one pixel per thread of a 256-thread workgroup");
static_assert(MS_MAXR + 1 <= 127, "the capped vertical distance is stored in a signed byte");

// Column pass.  A thread owns rows [y0, y0 + MS_CH) of one column.  It walks down from y0 - R counting the rows since the last inside
// and the last outside pixel (cap = R + 1 = "none within R"; it starts at cap, so the frame border is neither) and keeps the counts of
// its own rows in registers - the sign says which set a pixel is in, so nothing is loaded twice -, then walks up from y0 + MS_CH - 1 + R
// and stores the smaller of the two directions: R + MS_CH + R loads and MS_CH stores per thread.  The loads of a walk do not depend on
// one another, and the walk over the thread's own rows has a fixed trip count, so the compiler issues them in batches.
__global__ __launch_bounds__(256) void ms_column_kernel(const float* __restrict__ m, int8_t* __restrict__ v, int H, int W, float tau,
                                                         int cap, int tilesX, int chunks) {
    int64_t b = blockIdx.x;
    const int tx = (int)(b % tilesX);
    b /= tilesX;
    const int ch = (int)(b % chunks);
    const int64_t t = b / chunks;
    const int x = tx * MS_TILE + (int)threadIdx.x;
    if (x >= W) return;
    const int y0 = ch * MS_CH, y1 = min(y0 + MS_CH, H);   // (chunks = ceil(H / MS_CH): y0 < H)
    const int64_t base = t * H * W + x;
    const float* col = m + base;
    int8_t* vc = v + base;
    int ci = cap, co = cap;   // rows since the last inside / outside pixel
#pragma unroll 8
    for (int y = max(y0 - (cap - 1), 0); y < y0; ++y) {
        const bool in = col[(int64_t)y * W] > tau;   // (a NaN compares false: outside)
        ci = in ? 0 : min(ci + 1, cap);
        co = in ? min(co + 1, cap) : 0;
    }
    int down[MS_CH];   // +ci on an outside pixel (>= 1), -co on an inside pixel (<= -1)
#pragma unroll
    for (int k = 0; k < MS_CH; ++k) {
        const int y = min(y0 + k, H - 1);            // a row beyond the frame re-reads the last one: its count is never used
        const bool in = col[(int64_t)y * W] > tau;
        ci = in ? 0 : min(ci + 1, cap);
        co = in ? min(co + 1, cap) : 0;
        down[k] = in ? -co : ci;
    }
    ci = co = cap;
#pragma unroll 8
    for (int y = min(y1 - 1 + (cap - 1), H - 1); y >= y1; --y) {
        const bool in = col[(int64_t)y * W] > tau;
        ci = in ? 0 : min(ci + 1, cap);
        co = in ? min(co + 1, cap) : 0;
    }
#pragma unroll
    for (int k = MS_CH - 1; k >= 0; --k) {
        const int y = y0 + k;
        if (y < H) {   // (the same for every thread of the workgroup)
            const bool in = down[k] < 0;
            ci = in ? 0 : min(ci + 1, cap);
            co = in ? min(co + 1, cap) : 0;
            vc[(int64_t)y * W] = (int8_t)(in ? -min(co, -down[k]) : min(ci, down[k]));
        }
    }
}

struct MsParams {
    insv2v_mask_shape_plan_t p;
    float gf, f;   // g + f (formed in double, rounded once) and f
    int profile;
};

// Row pass.  A workgroup owns MS_TILE pixels of one row; si / so hold vi^2 / vo^2 of the segment and its halo, FAR outside the frame
// (there is no pixel of either set there).  (2 R + 1) taps of two LDS reads, an add and a min each.
__global__ __launch_bounds__(256) void ms_row_kernel(const int8_t* __restrict__ v, float* __restrict__ shaped, float* __restrict__ support,
                                                      int32_t* __restrict__ d2_out, int32_t* __restrict__ d2_in, int H, int W, int tilesX,
                                                      MsParams q) {
    __shared__ int si[MS_TILE + 2 * MS_MAXR], so[MS_TILE + 2 * MS_MAXR];
    int64_t b = blockIdx.x;
    const int tx = (int)(b % tilesX);
    const int64_t row = (b / tilesX) * W;   // (t * H + y) * W
    const int R = q.p.R, far = q.p.far, tid = (int)threadIdx.x;
    const int x0 = tx * MS_TILE;
    for (int i = tid; i < MS_TILE + 2 * R; i += 256) {
        const int gx = x0 - R + i;
        int a = far, o = far;
        if (gx >= 0 && gx < W) {
            const int c = v[row + gx];
            const int vi = max(c, 0), vo = max(-c, 0);
            a = vi * vi, o = vo * vo;
        }
        si[i] = a, so[i] = o;
    }
    __syncthreads();
    const int x = x0 + tid;
    if (x >= W) return;
    int a = far, o = far;
#pragma unroll 4
    for (int k = 0; k <= 2 * R; ++k) {
        const int dd = (k - R) * (k - R);
        a = min(a, dd + si[tid + k]);
        o = min(o, dd + so[tid + k]);
    }
    const int d2o = a > R * R ? far : a, d2i = o > R * R ? far : o;
    const bool inside = so[tid + R] > 0;
    const bool one = inside ? d2i >= q.p.in_one : d2o <= q.p.out_one;
    const bool zero = inside ? d2i <= q.p.in_zero : d2o >= q.p.out_zero;
    float val = one ? 1.f : 0.f;
    if (!one && !zero) {   // the ramp: D2 <= R^2 here, FAR never enters it
        const float s = inside ? 1.f - sqrtf((float)d2i) : sqrtf((float)d2o);
        const float u = (q.gf - s) / q.f;
        val = q.profile == INSV2V_MASK_PROFILE_SMOOTH ? u * u * (3.f - 2.f * u) : u;
        val = fminf(fmaxf(val, 0x1p-126f), 0x1.fffffep-1f);   // never exactly 0 or 1 (a NaN, 0 / 0 of a feather below fp32's resolution, becomes 2^-126)
    }
    const int64_t i = row + x;
    shaped[i] = val;
    support[i] = val > 0.f ? 1.f : 0.f;
    if (d2_out) d2_out[i] = d2o;
    if (d2_in) d2_in[i] = d2i;
}

int64_t ms_tiles_x(int32_t W) { return ((int64_t)W + MS_TILE - 1) / MS_TILE; }
int64_t ms_chunks(int32_t H) { return ((int64_t)H + MS_CH - 1) / MS_CH; }
constexpr int64_t MS_MAX_ELEMS = (int64_t)1 << 40;   // no offset or byte count overflows int64
constexpr int64_t MS_MAX_GRID = 0x7fffffffll;
bool ms_sizes_ok(int32_t T, int32_t H, int32_t W) {
    if (T < 1 || H < 1 || W < 1) return false;
    if ((int64_t)H * W > MS_MAX_ELEMS / T) return false;
    return (int64_t)T * H <= MS_MAX_GRID / ms_tiles_x(W);   // the row pass has the larger grid: H rows against ceil(H / MS_CH) chunks
}

}   // namespace

extern "C" int insv2v_mask_shape_plan(float grow, float feather, insv2v_mask_shape_plan_t* out) {
    if (!out) return INSV2V_EINVAL;
    *out = plan_mask_shape(grow, feather);
    return out->rc;
}

extern "C" int64_t insv2v_mask_shape_workspace_bytes(int32_t T, int32_t H, int32_t W) {
    if (!ms_sizes_ok(T, H, W)) return INSV2V_EINVAL;
    return ((int64_t)T * H * W + 3) / 4 * 4;
}

extern "C" int insv2v_mask_shape(const insv2v_mask_shape_desc* d, insv2v_stream_t stream) {
    if (!d || !d->m || !d->shaped || !d->support || !d->workspace) return INSV2V_EINVAL;
    const int64_t need = insv2v_mask_shape_workspace_bytes(d->T, d->H, d->W);
    if (need <= 0 || d->workspace_bytes < need || ((uintptr_t)d->workspace & 3)) return INSV2V_EINVAL;
    if (!isfinite(d->threshold) || (d->profile != INSV2V_MASK_PROFILE_LINEAR && d->profile != INSV2V_MASK_PROFILE_SMOOTH)) return INSV2V_EINVAL;
    MsParams q;
    q.p = plan_mask_shape(d->grow, d->feather);
    if (q.p.rc != 0 || q.p.R > MS_MAXR) return INSV2V_EINVAL;
    q.gf = (float)((double)d->grow + (double)d->feather), q.f = d->feather, q.profile = d->profile;
    const uintptr_t n = (uintptr_t)d->T * d->H * d->W;
    struct Span { uintptr_t lo, n; };
    const Span sp[6] = {{(uintptr_t)d->m, n * 4}, {(uintptr_t)d->shaped, n * 4}, {(uintptr_t)d->support, n * 4},
                        {(uintptr_t)d->d2_out, d->d2_out ? n * 4 : 0}, {(uintptr_t)d->d2_in, d->d2_in ? n * 4 : 0}, {(uintptr_t)d->workspace, (uintptr_t)need}};
    for (int i = 1; i < 6; ++i)   // every output against m and the outputs before it
        for (int j = 0; j < i; ++j)
            if (sp[i].n && sp[j].n && sp[i].lo < sp[j].lo + sp[j].n && sp[j].lo < sp[i].lo + sp[i].n) return INSV2V_EINVAL;
    const int tilesX = (int)ms_tiles_x(d->W), chunks = (int)ms_chunks(d->H);
    int8_t* v = (int8_t*)d->workspace;
    hipLaunchKernelGGL(ms_column_kernel, dim3((unsigned)((int64_t)d->T * chunks * tilesX)), dim3(256), 0, as_stream(stream), d->m, v, (int)d->H,
                       (int)d->W, d->threshold, q.p.R + 1, tilesX, chunks);
    if (int e = launch_status()) return e;
    hipLaunchKernelGGL(ms_row_kernel, dim3((unsigned)((int64_t)d->T * d->H * tilesX)), dim3(256), 0, as_stream(stream), (const int8_t*)v, d->shaped,
                       d->support, d->d2_out, d->d2_in, (int)d->H, (int)d->W, tilesX, q);
    return launch_status();
}
