// Mask estimation from the prompt: the kernels behind InferenceIP2PVideo.estimate_mask.  All of them are
// bandwidth- or launch-bound (a few hundred KB per call at 16 x 32 x 48 latents); none needs the matrix cores.
//   insv2v_build_unet_input_noised   the 3-branch UNet input of the source latent noised to a level, the noise a tensor or a seeded stream
//   insv2v_eps_absdiff_accum         acc (= | +=) scale * sum_c |eps3 - eps2| from the runner's channels-last output
//   insv2v_automask_finish           mean -> normalise -> smooth -> threshold -> dilate -> image-resolution mask
#include "common.h"
#include "rng.h"

// One thread per pixel (f,y,x) of the chunk: the noised latent is the same in the three branches, so its four channels are formed once
// (seeded: four elements of the stream, each generated on its own) and written three times.  The fp16 values are those of
// insv2v_add_noise (+ insv2v_randn) followed by insv2v_build_unet_input: noised_f and rng_normal_at are the shared expressions.
__global__ __launch_bounds__(256) void build_unet_input_noised_kernel(const float* __restrict__ z, const float* __restrict__ cond,
                                                                      const float* __restrict__ noise, half_t* __restrict__ out,
                                                                      float* __restrict__ t_out, float timestep, float ka, float kb,
                                                                      int64_t seed, int64_t stream, int F, int h, int w, int ldo,
                                                                      int64_t branch_rows, int t_stride) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over [F,h,w]
    const int64_t plane = (int64_t)h * w, total = (int64_t)F * plane;
    if (i < 3 && t_out) t_out[i * t_stride] = timestep;
    if (i >= total) return;
    const int64_t f = i / plane;
    const int64_t base = f * 4 * plane + (i - f * plane);         // element (f, 0, y, x) of [F,4,h,w]
    half_t lat[4], cnd[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int64_t e = base + c * plane;
        const float n = noise ? noise[e] : rng_normal_at(seed, stream, e);
        lat[c] = (half_t)noised_f(ka, z[e], kb, n);
        cnd[c] = (half_t)cond[e];
    }
#pragma unroll
    for (int br = 0; br < 3; ++br) {
        half_t* o = out + ((int64_t)br * branch_rows + i) * ldo;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            o[c] = lat[c];
            o[4 + c] = br > 0 ? cnd[c] : (half_t)0.f;
        }
        for (int c = 8; c < ldo; ++c) o[c] = (half_t)0.f;
    }
}
extern "C" int insv2v_build_unet_input_noised(const float* latent, const float* img_cond, const float* noise, void* out, float* t_out,
                                              float timestep, float ka, float kb, int64_t seed, int64_t noise_stream, int32_t seeded,
                                              int32_t F, int32_t h, int32_t w, int32_t ldo, int64_t branch_rows, int32_t t_stride,
                                              insv2v_stream_t stream) {
    if (!latent || !img_cond || !out || F <= 0 || h <= 0 || w <= 0 || ldo < 8 || (seeded != 0 && seeded != 1)) return INSV2V_EINVAL;
    if ((noise != nullptr) == (seeded != 0)) return INSV2V_EINVAL;   // one source of noise: a tensor or the stream, never both, never none
    const int64_t total = (int64_t)F * h * w;
    if (branch_rows == 0) branch_rows = total;
    if (t_stride == 0) t_stride = 1;
    if (branch_rows < total || t_stride < 0) return INSV2V_EINVAL;
    const int64_t grid = (total + 255) / 256;
    if (grid > 0x7fffffffll) return INSV2V_EINVAL;
    hipLaunchKernelGGL(build_unet_input_noised_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), latent, img_cond, noise,
                       (half_t*)out, t_out, timestep, ka, kb, seed, noise_stream, F, h, w, ldo, branch_rows, t_stride);
    return launch_status();
}

// One thread per pixel: its four channels are ONE 16-byte load from branch 1 and one from branch 2 (branch 0 and the other clips of a
// stack are never touched).  Summation order, which the fp32 emulation of the tests follows:
//   inside a pixel   s = (|d0| + |d1|) + (|d2| + |d3|), d_c = eps3_c - eps2_c
//   across draws     acc = fma(scale, s, acc) in the order of the calls (one rounding per draw); the first draw writes scale * s
__global__ __launch_bounds__(256) void eps_absdiff_accum_kernel(const float* __restrict__ eps, float* __restrict__ acc, int64_t total,
                                                                int64_t bs, float scale, int accumulate) {
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;   // over [F,h,w]
    if (pix >= total) return;
    const float4 a = *(const float4*)(eps + bs + pix * 4);
    const float4 b = *(const float4*)(eps + 2 * bs + pix * 4);
    const float s = (fabsf(b.x - a.x) + fabsf(b.y - a.y)) + (fabsf(b.z - a.z) + fabsf(b.w - a.w));
    acc[pix] = accumulate ? fmaf(scale, s, acc[pix]) : scale * s;
}
extern "C" int insv2v_eps_absdiff_accum(const float* eps, float* acc, int32_t F, int32_t h, int32_t w, int64_t branch_stride, float scale,
                                        int32_t accumulate, insv2v_stream_t stream) {
    if (!eps || !acc || F <= 0 || h <= 0 || w <= 0 || branch_stride < 0 || (accumulate != 0 && accumulate != 1)) return INSV2V_EINVAL;
    const int64_t total = (int64_t)F * h * w;
    const int64_t bs = branch_stride > 0 ? branch_stride : total * 4;
    if (bs < total * 4 || (bs & 3) || ((uintptr_t)eps & 15)) return INSV2V_EINVAL;   // the 16-byte loads; branches do not overlap
    const int64_t grid = (total + 255) / 256;
    if (grid > 0x7fffffffll) return INSV2V_EINVAL;
    hipLaunchKernelGGL(eps_absdiff_accum_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), eps, acc, total, bs, scale,
                       (int)accumulate);
    return launch_status();
}

// ---- finish: three launches.
//   1  partial sums of raw: P = automask_parts(N) blocks of 256 threads, thread t of block b adds elements (b 256 + t) + k P 256 in the
//      order of k, the block reduces with block_sum256 -> workspace[b]
//   2  every block reduces the P partials again with block_sum256 (the same order in every block, so every block holds the same bits of
//      the mean), then soft = smooth(min(raw, r mean) / (r mean))
//   3  threshold, dilate, replicate to image resolution
// No floating-point atomics anywhere: the order of every sum is fixed by the geometry, two runs give the same bits.
#define AUTOMASK_MAX_PARTS 256
static inline int64_t automask_parts(int64_t N) {
    const int64_t p = (N + 1023) / 1024;
    return p < 1 ? 1 : (p > AUTOMASK_MAX_PARTS ? AUTOMASK_MAX_PARTS : p);
}
// sum over the 256 threads of a block, the same value in every thread: shuffles inside a wave, then the four waves in order
__device__ __forceinline__ float block_sum256(float v, float* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}
__global__ __launch_bounds__(256) void automask_partial_kernel(const float* __restrict__ raw, float* __restrict__ parts, int64_t N) {
    __shared__ float red[4];
    const int64_t stride = (int64_t)gridDim.x * 256;
    float s = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += stride) s += raw[i];
    s = block_sum256(s, red);
    if (threadIdx.x == 0) parts[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void automask_soft_kernel(const float* __restrict__ raw, const float* __restrict__ parts, int P,
                                                            float* __restrict__ soft, int T, int h, int w, float clamp_ratio, int smooth) {
    __shared__ float red[4];
    const float total = block_sum256((int)threadIdx.x < P ? parts[threadIdx.x] : 0.f, red);
    const int64_t plane = (int64_t)h * w, N = (int64_t)T * plane;
    const float cap = clamp_ratio * (total / (float)N);            // r * mean
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // over [T,h,w]
    if (i >= N) return;
    auto soft0 = [&](int64_t j) { return cap > 0.f ? fminf(raw[j], cap) / cap : 0.f; };   // mean == 0: no division, an empty mask
    if (!smooth) {
        soft[i] = soft0(i);
        return;
    }
    const int t = (int)(i / plane);
    const int64_t r = i - (int64_t)t * plane;
    const int y = (int)(r / w), x = (int)(r - (int64_t)y * w);
    // edges replicated: a clamped index.  Every weight is a power of two, so the order below is exact up to the additions.
    const int64_t tm = (int64_t)(t > 0 ? t - 1 : 0) * plane, t0 = (int64_t)t * plane, tp = (int64_t)(t < T - 1 ? t + 1 : T - 1) * plane;
    const int ys[3] = {y > 0 ? y - 1 : 0, y, y < h - 1 ? y + 1 : h - 1};
    const int xs[3] = {x > 0 ? x - 1 : 0, x, x < w - 1 ? x + 1 : w - 1};
    float rows[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float v[3];
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const int64_t o = (int64_t)ys[a] * w + xs[b];
            v[b] = ((soft0(tm + o) + soft0(tp + o)) + 2.f * soft0(t0 + o)) * 0.25f;   // temporal [1,2,1]/4 first
        }
        rows[a] = (v[0] + v[2]) + 2.f * v[1];
    }
    soft[i] = ((rows[0] + rows[2]) + 2.f * rows[1]) * 0.0625f;                          // then spatial [1,2,1] x [1,2,1] / 16
}
// one thread per latent cell: max over the (2 dilate + 1)^2 square of (soft > threshold) inside the frame, the cell's 8 x 8 image pixels
// as two 16-byte stores per row
__global__ __launch_bounds__(256) void automask_mask_kernel(const float* __restrict__ soft, float* __restrict__ mask_latent,
                                                            float* __restrict__ mask, int64_t N, int h, int w, float threshold, int dilate) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;     // over [T,h,w]
    if (i >= N) return;
    const int64_t plane = (int64_t)h * w;
    const int64_t t = i / plane, r = i - t * plane;
    const int y = (int)(r / w), x = (int)(r - (int64_t)y * w);
    const int y0 = max(y - dilate, 0), y1 = min(y + dilate, h - 1), x0 = max(x - dilate, 0), x1 = min(x + dilate, w - 1);
    float m = 0.f;
    for (int yy = y0; yy <= y1 && m == 0.f; ++yy)
        for (int xx = x0; xx <= x1; ++xx)
            if (soft[t * plane + (int64_t)yy * w + xx] > threshold) { m = 1.f; break; }
    mask_latent[i] = m;
    const float4 v = make_float4(m, m, m, m);
    float* o = mask + ((t * h + y) * 8) * ((int64_t)w * 8) + (int64_t)x * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        *(float4*)(o + (int64_t)j * w * 8) = v;
        *(float4*)(o + (int64_t)j * w * 8 + 4) = v;
    }
}
extern "C" int64_t insv2v_automask_workspace_bytes(int32_t T, int32_t h, int32_t w) {
    if (T <= 0 || h <= 0 || w <= 0) return INSV2V_EINVAL;
    return automask_parts((int64_t)T * h * w) * (int64_t)sizeof(float);
}
extern "C" int insv2v_automask_finish(const float* raw, float* soft, float* mask_latent, float* mask, void* workspace, int64_t workspace_bytes,
                                      int32_t T, int32_t h, int32_t w, float clamp_ratio, float threshold, int32_t smooth, int32_t dilate,
                                      insv2v_stream_t stream) {
    if (!raw || !soft || !mask_latent || !mask || !workspace || T <= 0 || h <= 0 || w <= 0) return INSV2V_EINVAL;
    if (!(threshold > 0.f && threshold < 1.f) || !(clamp_ratio > 0.f) || dilate < 0 || (smooth != 0 && smooth != 1)) return INSV2V_EINVAL;   // (NaN fails both)
    if (((uintptr_t)mask & 15) || ((uintptr_t)workspace & 3)) return INSV2V_EINVAL;
    const int64_t N = (int64_t)T * h * w, P = automask_parts(N);
    if (workspace_bytes < P * (int64_t)sizeof(float)) return INSV2V_EINVAL;
    const uintptr_t bytes = (uintptr_t)N * sizeof(float);
    auto overlap = [bytes](const void* a, const void* b) { return (uintptr_t)a < (uintptr_t)b + bytes && (uintptr_t)b < (uintptr_t)a + bytes; };
    // raw's neighbours are read while soft is written, soft's while mask_latent is
    if (overlap(raw, soft) || overlap(soft, mask_latent) || overlap(raw, mask_latent)) return INSV2V_EINVAL;
    const int64_t grid = (N + 255) / 256;
    if (grid > 0x7fffffffll) return INSV2V_EINVAL;
    float* parts = (float*)workspace;
    hipLaunchKernelGGL(automask_partial_kernel, dim3((unsigned)P), dim3(256), 0, as_stream(stream), raw, parts, N);
    hipLaunchKernelGGL(automask_soft_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), raw, (const float*)parts, (int)P, soft,
                       T, h, w, clamp_ratio, (int)smooth);
    hipLaunchKernelGGL(automask_mask_kernel, dim3((unsigned)grid), dim3(256), 0, as_stream(stream), (const float*)soft, mask_latent, mask, N,
                       h, w, threshold, (int)dilate);
    return launch_status();
}
