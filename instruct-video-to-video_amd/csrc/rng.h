// Counter-based noise (ABI 14; the stream is the public contract documented in include/insv2v_hip.h, "seeded noise"): Philox4x32-10
// keyed by the seed, counter = (block, stream id), element i of a stream = output word i & 3 of block i >> 2, normals by Box-Muller on
// the word pairs (0,1) and (2,3) of a block.  ONE copy, included wherever noise is produced: insv2v_randn, the scheduler step and the
// VAE posterior sample call the same functions, so a value generated in place is bit-identical to the same element of insv2v_randn.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct rng_words { uint32_t w[4]; };

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the 128-bit block of (seed, stream, block).
__device__ __forceinline__ rng_words rng_philox_block(int64_t seed, int64_t stream, uint64_t block) {
    uint32_t k0 = (uint32_t)(uint64_t)seed, k1 = (uint32_t)((uint64_t)seed >> 32);
    uint32_t c0 = (uint32_t)block, c1 = (uint32_t)(block >> 32), c2 = (uint32_t)(uint64_t)stream, c3 = (uint32_t)((uint64_t)stream >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;   // (the bump after the last round is dead code)
    }
    return rng_words{{c0, c1, c2, c3}};
}

// Box-Muller on one pair of words: u = ((word >> 8) + 0.5) 2^-24, z0 = r cos(2 pi u1), z1 = r sin(2 pi u1), r = sqrt(-2 ln u0).
// (word >> 8) + 0.5 = (2 m + 1) / 2 has 25 significant bits once m >= 2^23, one more than fp32 holds, so neither u is formed as a
// float beyond that: ln u0 is taken through log1p of the exact complement 1 - u0 = (2^25 - (2 m + 1)) 2^-25 (< 2^24 there), and the
// angle is reduced by half a turn in integers (sin / cos of pi (x + 1) = - sin / cos of pi x).  Every float below is then an exact
// image of its word; what is left is the rounding of logf / log1pf, sqrtf and sincospif ("Seeded noise").
__device__ __forceinline__ void rng_box_muller(uint32_t w0, uint32_t w1, float& z0, float& z1) {
#pragma clang fp contract(off)
    const uint32_t a = 2u * (w0 >> 8) + 1u;                 // u0 = a 2^-25, a odd in [1, 2^25)
    const float ln_u0 = a < (1u << 24) ? logf((float)a * 0x1p-25f) : log1pf(-(float)((1u << 25) - a) * 0x1p-25f);
    const float r = sqrtf(-2.0f * ln_u0);
    const uint32_t b = 2u * (w1 >> 8) + 1u;                 // 2 u1 = b 2^-24 in (0, 2)
    float s, c;
    sincospif((float)(b & 0xffffffu) * 0x1p-24f, &s, &c);
    if (b >> 24) { s = -s; c = -c; }
    z0 = r * c;
    z1 = r * s;
}

// the four normals of a block
__device__ __forceinline__ void rng_normal4(const rng_words& q, float z[4]) {
    rng_box_muller(q.w[0], q.w[1], z[0], z[1]);
    rng_box_muller(q.w[2], q.w[3], z[2], z[3]);
}

// element `index` of the normal stream, generated on its own (one block, one Box-Muller pair)
__device__ __forceinline__ float rng_normal_at(int64_t seed, int64_t stream, int64_t index) {
    const rng_words q = rng_philox_block(seed, stream, (uint64_t)index >> 2);
    const int j = (int)(index & 3);
    float z0, z1;
    rng_box_muller(j & 2 ? q.w[2] : q.w[0], j & 2 ? q.w[3] : q.w[1], z0, z1);
    return j & 1 ? z1 : z0;
}
