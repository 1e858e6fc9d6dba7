// insv2v_gemm: fp16 MFMA GEMM / implicit-GEMM 3x3 convolution with fused epilogue.
//
// Roofline: MFMA-bound by FLOPs, in practice bound by the L2->LDS operand stream (profiles/r01_gemm_decomposition.txt).
// One workgroup = WM x WN (x KG) waves computes a BM x BN output tile with v_mfma_f32_32x32x16_f16 (default: 8 waves as
// 4 x 2, 128 x 128 tile, 2 workgroups per CU); the MFMA "A" operand is the weight fragment (rows = output channels n) and
// the "B" operand the activation fragment (cols = tokens m), so each lane ends up with 4 CONSECUTIVE output channels of
// one token.
//
// K is consumed in 64-wide slices through an LDS ring filled by LDS-DMA
// (buffer_load_dwordx4 ... lds: HBM/L2 -> LDS without a VGPR round trip and without ds_write
// traffic, which measured as the limiter of a register-staged version).  Addresses are
// SRD base + per-lane 32-bit byte offset (loop invariant) + wave-uniform scalar slice offset, so
// the K loop carries almost no address arithmetic; out-of-range rows, conv zero padding and the
// K tail use an offset beyond the descriptor's range, for which the hardware returns zeros.  LDS rows are
// 128 B (64 halfs), unpadded, with the 16-byte chunk index XOR-swizzled by ((row>>1)&7):
// the DMA writes lane-linearly, so the swizzle is applied to the per-lane SOURCE address and
// again on the fragment read, which makes every ds_read_b128 of a 32-row fragment
// conflict-free.
// STAGES=2: slices 0,1 requested up front; then wait(slice t) -> barrier -> issue slice t+1 -> MFMA slice t  (2 workgroups/CU)
// STAGES>2: counted vmcnt keeps S-2 slices in flight across the barrier (kept for A/B measurement:
// LDS capacity, not prefetch depth, limits the bytes in flight, so deeper rings did not pay).
// Tile ids are rasterised XCD-aware in groups of 8 tile rows (8 x 8 patches per XCD) for L2 locality.
//
// In CONV3X3 mode the activation rows are gathered on the fly (tap-shifted pixels, zero
// fill at the border, optional nearest-x2 upsample and channel concat), so im2col, the
// upsampled tensor and torch.cat are never materialised in HBM.  Stride-1 convs whose output divides into
// 8x16 / 16x8 pixel patches go to conv_halo_kernel instead (input patch resident in LDS across the 9 taps).
//
// Epilogue (tile_epilogue): alpha, folded LayerNorm, bias, per-sample / per-frame row bias, SiLU / quick-GELU / GEGLU
// in registers; the fp32 tile is staged through the (now idle) LDS so global stores and residual loads are contiguous
// 16-byte chunks of whole output rows.  Bias / column sums / token statistics are parked in LDS before the K loop.
#include "common.h"
#include <algorithm>
#include "gemm_dma.h"
#include "gemm_plan.h"
static_assert(GEMM_BK == BK, "gemm_plan.h restates the K slice");
#include <type_traits>
#include <cstdlib>

typedef unsigned uint4r __attribute__((ext_vector_type(4)));  // 128-bit register operand of inline asm

struct RowInfo {  // per-thread metadata of one staged activation row
    int base;      // linear: m ; conv: nb*IH*IW (pixel index of the image's first pixel)
    int oh, ow;    // conv only (already multiplied by stride, minus pad)
    bool valid;
};

// Debug-only phase timer (tools/gemm_phase_prof.py builds a separate library with -DINSV2V_GEMM_PROF; the shipped
// library never contains it): thread 0 accumulates 100 MHz wall-clock ticks per phase of every interior workgroup.
#ifdef INSV2V_GEMM_PROF
__device__ unsigned long long g_prof[8];
#define PROF_MARK(i) do { if (tid == 0) prof_t[i] = wall_clock64(); } while (0)
#else
#define PROF_MARK(i) do { } while (0)
#endif

// Sum over the aligned group of W consecutive lanes (W = 4, 8, 16) on the VALU: quad_perm, quad_perm, row_half_mirror, row_mirror
template <int W>
__device__ __forceinline__ float lane_group_sum(float v) {
    static_assert(W == 4 || W == 8 || W == 16, "a DPP row is 16 lanes");
    auto dpp = [](float x, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xF, 0xF, true));
    };
    v += dpp(v, std::integral_constant<int, 0xB1>{});                 // lanes 1,0,3,2
    v += dpp(v, std::integral_constant<int, 0x4E>{});                 // lanes 2,3,0,1
    if (W >= 8) v += dpp(v, std::integral_constant<int, 0x141>{});    // row_half_mirror
    if (W >= 16) v += dpp(v, std::integral_constant<int, 0x140>{});   // row_mirror
    return v;
}

// Whether a workgroup's output takes the vectorised fp16 path of tile_epilogue (whole-launch property)
__device__ __forceinline__ bool fast_output_ok(const insv2v_gemm_desc& p, const char* Cb, const half_t* Rp, int oN) {
    const bool vec_ok = ((p.ldc & 7) == 0) && (((uintptr_t)Cb & (p.c_fp32 ? 31 : 15)) == 0) &&
                        (!Rp || (((p.ldr & 7) == 0) && (((uintptr_t)Rp & 15) == 0)));
    const bool res32 = !Rp || (int64_t)p.M * p.ldr * 2 < ((int64_t)1 << 31);
    return vec_ok && !p.c_fp32 && (oN & 7) == 0 && res32;
}

// Shared tile epilogue.  acc holds the wave's MI x NI fragments; grow(r) maps tile-local row r to the global output
// row (token / pixel index), rows_full says every row of the tile exists.  sBias / sCs / sStat are the LDS copies of
// bias, folded-LayerNorm column sums and per-row (mean, rstd) made by the caller before its K loop.
template <int WM, int WN, int MI, int NI, int KG, bool HAS_LN, class RowMap>
__device__ __forceinline__ void tile_epilogue(const insv2v_gemm_desc& p, floatx16 (&acc)[NI][MI], char* smem, const float* sBias,
                                              const float* sCs, const float2* sStat, int tid, int wm, int wn, int kg, int bn0,
                                              int z, int zs, bool rows_full, RowMap grow
#ifdef INSV2V_GEMM_PROF
                                              , unsigned long long* prof_t
#endif
) {
    constexpr int NWV = WM * WN * KG, NT = NWV * 64;
    constexpr int BM = WM * MI * 32, BN = WN * NI * 32;
    const int lane = tid & 63;
    const bool geglu = p.act == INSV2V_ACT_GEGLU;
    const int oN = geglu ? (p.N >> 1) : p.N;          // output columns
    const int on0 = geglu ? (bn0 >> 1) : bn0;         // first output column of this tile
    constexpr int CLD = BN + 4;                        // floats per staged row (fp32: one rounding, after the residual add)
    float* sC = (float*)smem;
    char* Cb = (char*)p.c + ((int64_t)z * p.c_bs + (int64_t)zs * p.M * p.ldc) * (p.c_fp32 ? 4 : 2);  // zs > 0 only for split-K partial slabs
    const half_t* Rp = p.residual ? (const half_t*)p.residual + z * p.r_bs : nullptr;
    if (KG > 1) {
        // partial sums of the K groups meet in the staging buffer: every lane of group g > 0 parks its
        // accumulators at the positions the SAME lane of group 0 owns, so no ordering beyond the barrier is needed
        for (int g = 1; g < KG; ++g) {
            if (kg == g) {
#pragma unroll
                for (int j = 0; j < MI; ++j)
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int q = 0; q < 4; ++q)
                            *(float4*)(sC + (wm * MI * 32 + j * 32 + (lane & 31)) * CLD + wn * NI * 32 + i * 32 + 8 * q + 4 * (lane >> 5)) =
                                make_float4(acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]);
            }
            __syncthreads();
            if (kg == 0) {
#pragma unroll
                for (int j = 0; j < MI; ++j)
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float4 t = *(const float4*)(sC + (wm * MI * 32 + j * 32 + (lane & 31)) * CLD + wn * NI * 32 + i * 32 + 8 * q + 4 * (lane >> 5));
                            acc[i][j][4 * q] += t.x; acc[i][j][4 * q + 1] += t.y; acc[i][j][4 * q + 2] += t.z; acc[i][j][4 * q + 3] += t.w;
                        }
            }
            if (g + 1 < KG) __syncthreads();
        }
    }
    typedef unsigned uint4e __attribute__((ext_vector_type(4)));
    const srd_t rRB = make_srd(p.row_bias ? (const void*)p.row_bias : (const void*)p.w);
    // whole-workgroup choice: 16-byte row-bias loads need N % 4 == 0, an aligned table and offsets below 2^31
    const bool rb_vec = p.row_bias && (p.N & 3) == 0 && (p.ld_rb & 3) == 0 && (((uintptr_t)p.row_bias & 15) == 0);
    if (KG == 1 || kg == 0) {
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        const int ml = wm * MI * 32 + j * 32 + (lane & 31);
        const int m = grow(ml);
        // Row bias (per-sample time embedding / per-frame positional-encoding table): 16-byte BUFFER loads whose offset is out of
        // range (-> zeros) where no bias applies.  A plain load inside `if (rb)` is a divergent branch per fragment quarter, and hipcc
        // waits vmcnt(0) at every join: 8 serial L2 round trips per thread in this epilogue (profiles/r02_epilogue_loads.txt).
        const float* rb = nullptr;
        unsigned rb_off = OOB_OFFSET;   // byte offset of this row's bias row; vector path only when N % 4 == 0
        if (p.row_bias && m < p.M) {
            int grp = m / p.rows_per_group;
            if (p.rb_mod > 0) grp %= p.rb_mod;
            rb = p.row_bias + (int64_t)grp * p.ld_rb;
            rb_off = (unsigned)(grp * (int)p.ld_rb * 4);
        }
        // all of this row's bias quarters at once (NI x 4 requests in flight; one per fragment quarter in the loop below was one
        // L2 round trip each)
        floatx4 rbv[NI][4];
        if (rb_vec) {
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int n = bn0 + wn * NI * 32 + i * 32 + 8 * q + 4 * (lane >> 5);
                    rbv[i][q] = __builtin_bit_cast(floatx4, (uint4e)__builtin_amdgcn_raw_buffer_load_b128(rRB, (rb && n + 3 < p.N) ? rb_off + (unsigned)(n * 4) : OOB_OFFSET, 0, 0));
                }
        }
        // folded LayerNorm: v = rstd*(alpha*acc - mean*col_sum[n]) (+ bias terms)
        float ln_m = 0.f, ln_r = 1.f;
        if (HAS_LN) { const float2 st = sStat[ml]; ln_m = st.x; ln_r = st.y; }
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (geglu && (i & 1)) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int nl = wn * NI * 32 + i * 32 + 8 * q + 4 * (lane >> 5);  // tile-local n of v[0]
                const int n = bn0 + nl;
                float v[4];
                const float4 bt = *(const float4*)(sBias + nl), ct = HAS_LN ? *(const float4*)(sCs + nl) : make_float4(0.f, 0.f, 0.f, 0.f);
                float bsum[4] = {bt.x, bt.y, bt.z, bt.w};
                const float cs[4] = {ct.x, ct.y, ct.z, ct.w};
                if (rb_vec) {
                    const floatx4 t = rbv[i][q];
                    bsum[0] += t[0]; bsum[1] += t[1]; bsum[2] += t[2]; bsum[3] += t[3];
                } else if (rb) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (n + e < p.N) bsum[e] += rb[n + e];
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = ln_r * (acc[i][j][4 * q + e] * p.alpha - ln_m * cs[e]) + bsum[e];
                int onl = nl;  // tile-local output column
                if (geglu) {
                    const float4 gbt = *(const float4*)(sBias + nl + 32), gct = HAS_LN ? *(const float4*)(sCs + nl + 32) : make_float4(0.f, 0.f, 0.f, 0.f);
                    float gb[4] = {gbt.x, gbt.y, gbt.z, gbt.w};
                    const float gcs[4] = {gct.x, gct.y, gct.z, gct.w};
                    if (rb_vec) {
                        const floatx4 t = rbv[(i + 1) % NI][q];   // the gate block is the next 32 channels: its own quarter q
                        gb[0] += t[0]; gb[1] += t[1]; gb[2] += t[2]; gb[3] += t[3];
                    } else if (rb && n + 35 < p.N) {
                        const float4 t = *(const float4*)(rb + n + 32);
                        gb[0] += t.x; gb[1] += t.y; gb[2] += t.z; gb[3] += t.w;
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        v[e] *= gelu_erf_f(ln_r * (acc[(i + 1) % NI][j][4 * q + e] * p.alpha - ln_m * gcs[e]) + gb[e]);
                    onl = (nl >> 6) * 32 + (nl & 31);
                } else if (p.act == INSV2V_ACT_SILU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = silu_f(v[e]);
                } else if (p.act == INSV2V_ACT_QUICK_GELU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = quick_gelu_f(v[e]);
                } else if (p.act >= INSV2V_ACT_RELU) {   // RAFT's small GEMMs (ReLU / sigmoid / tanh, oracle/raft.py)
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = act_raft_f(v[e], p.act);
                }
                *(float4*)(sC + ml * CLD + onl) = make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    }
    }
    PROF_MARK(3);
    __syncthreads();
    PROF_MARK(4);
    const int OW8 = (geglu ? BN / 2 : BN) / 8;  // 16-byte chunks per staged output row
    const bool vec_ok = ((p.ldc & 7) == 0) && (((uintptr_t)Cb & (p.c_fp32 ? 31 : 15)) == 0) &&
                        (!Rp || (((p.ldr & 7) == 0) && (((uintptr_t)Rp & 15) == 0)));
    // fast path: fp16 tile whose valid columns are whole 16-byte chunks -> fully unrolled, constant divisors, ALL residual loads
    // issued up front.  Edge tiles (last rows, N = 320 with 128-wide tiles: every third tile) take it too: chunks outside the
    // problem load with an out-of-range buffer offset and skip the store.  (They used to fall to the generic loop below, whose
    // per-chunk residual load + wait made them - and with them the whole launch - 4-8 memory round trips longer.)
    if (fast_output_ok(p, Cb, Rp, oN)) {
        const srd_t rRes = make_srd(Rp ? (const void*)Rp : (const void*)p.w);
        auto copy_rows = [&](auto w8_tag) {
            constexpr int W8 = decltype(w8_tag)::value;
            constexpr int ITERS = (BM * W8) / NT;
            static_assert((BM * W8) % NT == 0, "staged tile must divide evenly over the workgroup");
            half8 rv[ITERS];
            bool ok[ITERS];
            int mrow[ITERS];
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                const int idx = tid + it * NT, row = idx / W8, ch = idx % W8;
                mrow[it] = grow(row);
                ok[it] = (rows_full || mrow[it] < p.M) && on0 + ch * 8 + 8 <= oN;
                if (Rp) rv[it] = __builtin_bit_cast(half8, (uint4e)__builtin_amdgcn_raw_buffer_load_b128(
                            rRes, ok[it] ? (unsigned)((mrow[it] * (int)p.ldr + on0 + ch * 8) * 2) : OOB_OFFSET, 0, 0));
            }
#pragma unroll
            for (int it = 0; it < ITERS; ++it) {
                const int idx = tid + it * NT, row = idx / W8, ch = idx % W8;
                const float4 f0 = *(const float4*)(sC + row * CLD + ch * 8);
                const float4 f1 = *(const float4*)(sC + row * CLD + ch * 8 + 4);
                const float fv[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
                half8 hv;
#pragma unroll
                for (int e = 0; e < 8; ++e) hv[e] = (half_t)(Rp ? fv[e] + (float)rv[it][e] : fv[e]);
                if (ok[it]) *(half8*)((half_t*)Cb + (int64_t)mrow[it] * p.ldc + on0 + ch * 8) = hv;
                if constexpr (W8 == 4 || W8 == 8 || W8 == 16) {
                    // LayerNorm statistics of the NEXT op from the values just stored (fp16-rounded, after the residual add): the W8
                    // lanes holding one row's chunks reduce on the VALU; one (sum, sum of squares) pair per row and column tile
                    if (p.stats_out) {
                        float s1 = 0.f, s2 = 0.f;
#pragma unroll
                        for (int e = 0; e < 8; ++e) { const float x = ok[it] ? (float)hv[e] : 0.f; s1 += x; s2 = fmaf(x, x, s2); }
                        s1 = lane_group_sum<W8>(s1);
                        s2 = lane_group_sum<W8>(s2);
                        if (ch == 0 && (rows_full || mrow[it] < p.M))
                            *(float2*)(p.stats_out + ((int64_t)(bn0 / BN) * p.M + mrow[it]) * 2) = make_float2(s1, s2);
                    }
                }
            }
        };
        if (geglu) copy_rows(std::integral_constant<int, BN / 16>{});
        else copy_rows(std::integral_constant<int, BN / 8>{});
#ifdef INSV2V_GEMM_PROF
        wait_vmcnt<0>();
        PROF_MARK(5);
        if (tid == 0) {
            for (int i = 0; i < 5; ++i) atomicAdd(&g_prof[i], prof_t[i + 1] - prof_t[i]);
            atomicAdd(&g_prof[5], 1ull);
        }
#endif
        return;
    }
    for (int idx = tid; idx < BM * OW8; idx += NT) {
        const int row = idx / OW8, ch = idx - row * OW8;
        const int m = grow(row), on = on0 + ch * 8;
        if (m >= p.M || on >= oN) continue;
        const float4 f0 = *(const float4*)(sC + row * CLD + ch * 8);
        const float4 f1 = *(const float4*)(sC + row * CLD + ch * 8 + 4);
        float fv[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
        if (p.c_fp32) {  // conv_out / VAE moments / time embedding / split-K partial slabs
            float* dst32 = (float*)Cb + (int64_t)m * p.ldc + on;
            if (Rp) {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (on + e < oN) fv[e] += (float)Rp[(int64_t)m * p.ldr + on + e];
            }
            if (vec_ok && on + 7 < oN) {
                *(float4*)dst32 = make_float4(fv[0], fv[1], fv[2], fv[3]);
                *(float4*)(dst32 + 4) = make_float4(fv[4], fv[5], fv[6], fv[7]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (on + e < oN) dst32[e] = fv[e];
            }
            continue;
        }
        half_t* dst = (half_t*)Cb + (int64_t)m * p.ldc + on;
        if (vec_ok && on + 7 < oN) {
            half8 hv;
            if (Rp) {
                const half8 rv = *(const half8*)(Rp + (int64_t)m * p.ldr + on);
#pragma unroll
                for (int e = 0; e < 8; ++e) hv[e] = (half_t)(fv[e] + (float)rv[e]);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) hv[e] = (half_t)fv[e];
            }
            *(half8*)dst = hv;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (on + e < oN) dst[e] = (half_t)(fv[e] + (Rp ? (float)Rp[(int64_t)m * p.ldr + on + e] : 0.f));
        }
    }
}

// WM x WN waves, each owning MI x NI fragments of 32x32: BM = WM*MI*32 tokens, BN = WN*NI*32 channels.
// KG > 1: KG groups of WM x WN waves share the tile; group g multiplies the g-th 64/KG-wide part of every K slice
// (same DMA ring, 1/KG of the LDS fragment reads per MFMA) and the partial sums meet in LDS before the epilogue.
template <int WM, int WN, int MI, int NI, int MODE, int STAGES, int KG = 1>
__global__ __launch_bounds__(WM * WN * KG * 64) void gemm_kernel(insv2v_gemm_desc p) {
    constexpr int NWV = WM * WN * KG;
    constexpr int BM = WM * MI * 32, BN = WN * NI * 32;
    constexpr int LD = BK;                          // halfs per LDS row (128 B, unpadded, XOR-swizzled chunks)
    constexpr int RPP = 8 * NWV;                    // tile rows filled by one DMA instruction of every wave
    constexpr int RA = BM / RPP, RW = BN / RPP;     // DMA instructions per wave per slice (activations / weights)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    half_t* sA = (half_t*)smem;                     // [STAGES][BM][LD]
    half_t* sW = sA + STAGES * BM * LD;             // [STAGES][BN][LD]
    constexpr int RING_B = STAGES * (BM + BN) * BK * 2, STAGE_B = BM * (BN + 4) * 4;
    float* sBias = (float*)(smem + (RING_B > STAGE_B ? RING_B : STAGE_B));  // [BN] bias, [BN] col_sum, [BM] (mean, rstd)
    float* sCs = sBias + BN;
    float2* sStat = (float2*)(sCs + BN);

    const int tid = threadIdx.x, lane = tid & 63;
#ifdef INSV2V_GEMM_PROF
    unsigned long long prof_t[6];
#endif
    PROF_MARK(0);
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kg = wid / (WM * WN), wl = wid % (WM * WN);
    const int wm = wl / WN, wn = wl % WN;
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = (p.M + BM - 1) / BM;
    const int bid = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    // Rasterisation: after the XCD remap each XCD runs a contiguous run of ~64 tile ids at a time (32 CUs x 2
    // workgroups).  Ids walk groups of GROUP_M tile rows column by column, so such a run is a ~8 x 8 patch that
    // needs 8 + 8 operand panels from beyond its L2 instead of 1 + 64 (what row-major order costs when N is wide).
    constexpr int GROUP_M = 8;
    const int per_group = GROUP_M * tiles_n;
    const int gidx = bid / per_group, first_m = gidx * GROUP_M;
    const int gsz = min(GROUP_M, tiles_m - first_m), rin = bid - gidx * per_group;
    const int tn = rin / gsz, tm = first_m + rin - tn * gsz;
    const int bm0 = tm * BM, bn0 = tn * BN;
    const int z = blockIdx.y;

    const half_t* A = (const half_t*)p.a + z * p.a_bs;
    const half_t* A2 = p.a2 ? (const half_t*)p.a2 + z * p.a_bs : A;
    const half_t* Wp = (const half_t*)p.w + z * p.w_bs;
    const srd_t rA = make_srd(A), rA2 = make_srd(A2), rW = make_srd(Wp);

    // staging map: DMA instruction i of wave `wid` fills the 8-row group (i*NWV + wid):
    // row = group*8 + lane/8, LDS chunk slot lane%8, i.e. exactly lane-linear 1 KiB per instruction;
    // the lane fetches the LOGICAL chunk slot ^ ((row>>1)&7) (swizzle on the source side).
    const int crow = wid * 8 + (lane >> 3);
    const int cslot = lane & 7;

    RowInfo ri[RA];
    int achunk[RA];
    unsigned aoff1[RA], aoff2[RA];  // per-lane byte offsets into source 1 / 2 (linear: final; conv: un-shifted tap)
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int row = crow + RPP * i;
        achunk[i] = cslot ^ ((row >> 1) & 7);
        const int m = bm0 + row;
        ri[i].valid = m < p.M;
        if (MODE == INSV2V_MODE_LINEAR) {
            ri[i].base = m;
            ri[i].oh = ri[i].ow = 0;
            aoff1[i] = ri[i].valid ? (unsigned)(((int64_t)m * p.lda + achunk[i] * 8) * 2) : OOB_OFFSET;
            aoff2[i] = ri[i].valid ? (unsigned)(((int64_t)m * p.lda2 + achunk[i] * 8) * 2) : OOB_OFFSET;
        } else {
            int mm = ri[i].valid ? m : 0;
            int ow = mm % p.OW, t = mm / p.OW;
            int oh = t % p.OH, nb = t / p.OH;
            ri[i].base = nb * p.IH * p.IW;
            ri[i].oh = oh * p.stride - p.pad_t;
            ri[i].ow = ow * p.stride - p.pad_l;
            const int64_t pix = (int64_t)ri[i].base + (int64_t)ri[i].oh * p.IW + ri[i].ow;  // may be < 0 at the border
            aoff1[i] = (unsigned)((pix * p.lda + achunk[i] * 8) * 2);
            aoff2[i] = (unsigned)((pix * p.lda2 + achunk[i] * 8) * 2);
        }
    }
    int wchunk[RW];
    unsigned woff[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        const int row = crow + RPP * i;
        wchunk[i] = cslot ^ ((row >> 1) & 7);
        const int n = bn0 + row;
        woff[i] = n < p.N ? (unsigned)(((int64_t)n * p.ldw + wchunk[i] * 8) * 2) : OOB_OFFSET;
    }

    // split-K: workgroup blockIdx.z consumes slices [kt0, kt0 + nk) and writes an fp32 partial tile
    const int nk_total = (p.K + BK - 1) / BK;
    const int zs = blockIdx.z, nsplit = p.split_k > 1 ? p.split_k : 1;

    // (Requesting this thread's residual pieces here, before the K loop, was tried in round 2: correct, +28 VGPRs, and no faster -
    // out-proj 73 728 x 320 x 320 46 vs 43-44 us, 3-stream UNet step unchanged - the residual round trip is not what a short-K tile
    // waits for.  tools/gemm_phase_prof.py shows the phases.)
    const int nk_per = (nk_total + nsplit - 1) / nsplit;
    const int kt0 = zs * nk_per;
    const int nk = max(0, min(nk_per, nk_total - kt0));
    const int IHu = p.upsample ? p.OH : p.IH, IWu = p.upsample ? p.OW : p.IW;   // upsample: the (possibly cropped) nearest-x2 image IS the output extent (stride 1, pad 1)

    // Slices are requested in increasing order: everything slice-dependent is a wave-uniform scalar
    // kept in a cursor (no division, no 64-bit arithmetic in the loop).
    struct Cursor {
        int k0, kh, kw, ci0;
    } cur_k = {kt0 * BK, 0, 0, 0};
    if (MODE != INSV2V_MODE_LINEAR) {
        const int tap = cur_k.k0 / p.Cin;  // once per workgroup
        cur_k.ci0 = cur_k.k0 - tap * p.Cin;
        cur_k.kh = tap / 3;
        cur_k.kw = tap - cur_k.kh * 3;
    }
    auto advance = [&]() {
        cur_k.k0 += BK;
        if (MODE != INSV2V_MODE_LINEAR) {
            cur_k.ci0 += BK;
            if (cur_k.ci0 >= p.Cin) {
                cur_k.ci0 = 0;
                if (++cur_k.kw == 3) { cur_k.kw = 0; ++cur_k.kh; }
            }
        }
    };
    auto issue_slice = [&](int buf) {
        char* a = (char*)(sA + buf * BM * LD) + wid * 1024;
        char* w = (char*)(sW + buf * BN * LD) + wid * 1024;
        const bool ktail = cur_k.k0 + BK > p.K;  // only the last slice of a K that is not a multiple of 64
        if (MODE == INSV2V_MODE_LINEAR) {
            const bool second = p.k_split > 0 && cur_k.k0 >= p.k_split;
            const int soff = (second ? cur_k.k0 - p.k_split : cur_k.k0) * 2;
#pragma unroll
            for (int i = 0; i < RA; ++i) {
                unsigned v = second ? aoff2[i] : aoff1[i];
                if (ktail && cur_k.k0 + achunk[i] * 8 >= p.K) v = OOB_OFFSET;
                dma16(second ? rA2 : rA, v, soff, a + i * (NWV * 1024));
            }
        } else {
            const bool second = p.k_split > 0 && cur_k.ci0 >= p.k_split;
            const int ld = (int)(second ? p.lda2 : p.lda);
            const int cl = second ? cur_k.ci0 - p.k_split : cur_k.ci0;
            const int tapoff = ((cur_k.kh * p.IW + cur_k.kw) * ld + cl) * 2;  // uniform byte shift of this tap / channel block
#pragma unroll
            for (int i = 0; i < RA; ++i) {
                const int ih = ri[i].oh + cur_k.kh, iw = ri[i].ow + cur_k.kw;
                const bool ok = ri[i].valid && (unsigned)ih < (unsigned)IHu && (unsigned)iw < (unsigned)IWu;
                unsigned v;
                if (p.upsample)  // nearest x2: source pixel (ih>>1, iw>>1); not separable per tap
                    v = (unsigned)((((ri[i].base + (ih >> 1) * p.IW + (iw >> 1)) * ld) + cl + achunk[i] * 8) * 2);
                else
                    v = (second ? aoff2[i] : aoff1[i]) + (unsigned)tapoff;
                dma16(second ? rA2 : rA, ok ? v : OOB_OFFSET, 0, a + i * (NWV * 1024));
            }
        }
        const int wsoff = cur_k.k0 * 2;
#pragma unroll
        for (int i = 0; i < RW; ++i) {
            unsigned v = woff[i];
            if (ktail && cur_k.k0 + wchunk[i] * 8 >= p.K) v = OOB_OFFSET;
            dma16(rW, v, wsoff, w + i * (NWV * 1024));
        }
        advance();
    };

    floatx16 acc[NI][MI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int frow = lane & 31, fhalf = lane >> 5;
    auto compute = [&](int buf) {
        const half_t* a = sA + buf * BM * LD + (wm * MI * 32 + frow) * LD;
        const half_t* w = sW + buf * BN * LD + (wn * NI * 32 + frow) * LD;
        // swizzle term of this lane's fragment rows: rows differ by multiples of 32 across j/i, so
        // ((row>>1)&7) depends on frow only
        const int sw = (frow >> 1) & 7;
#pragma unroll
        for (int kq = 0; kq < BK / 16 / KG; ++kq) {
            const int kk = kg * (BK / 16 / KG) + kq;
            const int c = ((kk * 2 + fhalf) ^ sw) * 8;
            half8 fa[MI], fw[NI];
#pragma unroll
            for (int j = 0; j < MI; ++j) fa[j] = *(const half8*)(a + j * 32 * LD + c);
#pragma unroll
            for (int i = 0; i < NI; ++i) fw[i] = *(const half8*)(w + i * 32 * LD + c);
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < MI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[i], fa[j], acc[i][j], 0, 0, 0);
        }
    };

    // S-stage ring: slices kt+1 .. kt+S-2 stay in flight (counted vmcnt) while slice kt is consumed;
    // slice kt+S-1 is issued right after the barrier into the buffer slice kt-1 just vacated.
    // Epilogue vectors (bias, folded-LayerNorm column sums, per-token mean/rstd) are requested BEFORE the
    // first slices and parked in a small LDS area behind the ring/staging buffer, so the epilogue never
    // waits on a global load.  Out-of-range entries are neutral (0 / rstd 1).
    const bool ln = p.row_stats != nullptr;
    float pre_b = 0.f, pre_c = 0.f;
    float2 pre_s = make_float2(0.f, 1.f);
    if (tid < BN && bn0 + tid < p.N) {
        if (p.bias) pre_b = p.bias[bn0 + tid];
        if (ln) pre_c = p.col_sum[bn0 + tid];
    }
    if (tid < BM && ln && bm0 + tid < p.M) {
        if (p.stats_parts > 0) {  // partial sums written by the producing GEMM's epilogue, one pair per column tile
            float s1 = 0.f, s2 = 0.f;
            for (int j = 0; j < p.stats_parts; ++j) {
                const float2 t = ((const float2*)p.row_stats)[(int64_t)j * p.M + bm0 + tid];
                s1 += t.x; s2 += t.y;
            }
            const float mean = s1 / p.K;
            pre_s = make_float2(mean, rsqrtf(fmaxf(s2 / p.K - mean * mean, 0.f) + p.ln_eps));
        } else {
            pre_s = ((const float2*)p.row_stats)[bm0 + tid];
        }
    }

    constexpr int LPT = RA + RW;  // LDS-DMA instructions per wave per slice
    // The whole ring is requested up front (slices 0 .. STAGES-1): the first two slices' memory latencies overlap instead of
    // the second one starting only after the first has landed - one latency saved per tile, which matters for the many
    // short-K (5-20 slice) tiles.  From iteration 1 on, slice kt+STAGES-1 goes into the buffer slice kt-1 just vacated.
#pragma unroll
    for (int s = 0; s < STAGES; ++s)
        if (s < nk) issue_slice(s);
    if (tid < BN) { sBias[tid] = pre_b; sCs[tid] = pre_c; }
    if (tid < BM) sStat[tid] = pre_s;
    int cur = 0, nxt = STAGES - 1;
    for (int kt = 0; kt < nk; ++kt) {
        // younger slices allowed to stay in flight while slice kt is awaited
        const int behind = kt == 0 ? min(STAGES - 1, nk - 1) : min(STAGES - 2, nk - 1 - kt);
        if (behind <= 0) wait_vmcnt<0>();
        else if (behind == 1) wait_vmcnt<LPT>();
        else if (behind == 2) wait_vmcnt<2 * LPT>();
        else wait_vmcnt<3 * LPT>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#ifdef INSV2V_GEMM_PROF
        if (kt == 0) PROF_MARK(1);
#endif
        if (kt > 0 && kt + STAGES - 1 < nk) issue_slice(nxt);
        compute(cur);
        cur = (cur + 1 == STAGES) ? 0 : cur + 1;
        nxt = (nxt + 1 == STAGES) ? 0 : nxt + 1;
    }
    wait_vmcnt<0>();
    __syncthreads();
    PROF_MARK(2);

    // ---- epilogue ---------------------------------------------------------------------------------
    tile_epilogue<WM, WN, MI, NI, KG, true>(p, acc, smem, sBias, sCs, sStat, tid, wm, wn, kg, bn0, z, zs, bm0 + BM <= p.M,
                                            [&](int r) { return bm0 + r; }
#ifdef INSV2V_GEMM_PROF
                                            , prof_t
#endif
    );
}


// ------------------------------------------------------------------------------------------------------------
// conv_halo_kernel: stride-1 3x3 convolution whose output tile is a TH x TW pixel PATCH of one image (8x16 or 16x8 =
// 128 rows).  The 9 taps of a 64-channel block all read the same (TH+2)x(TW+2) input patch, so that patch is brought
// into LDS ONCE per channel block (<= 180 pixel rows x 128 B) and every tap's activation fragments are read from it at
// shifted rows; only the weight slices (BN x 64) stream per tap.  Compared with gathering a fresh 128-row activation
// slice per tap this cuts the L2->LDS operand stream of the K loop from 9 x 32 KB to 9 x 16 KB + 23 KB per channel
// block (0.58x) - the stream is what bounds the implicit-GEMM kernel (profiles/r01_gemm_decomposition.txt).
// K order is channel-block major, tap minor.  Nearest-x2 upsampling reads a (TH/2+2)x(TW/2+2) source patch; channel
// concat picks the source per channel block; zero padding = out-of-range DMA offsets.  2 workgroups / CU.
// GN = true: the input is the RAW tensor and p.gn_ab holds per-(sample, channel) (scale, shift): every thread applies
// y = act(x*scale + shift) to the 16 bytes of the patch it requested itself, in LDS, one tap after the piece was requested
// (the per-tap vmcnt(0) + barrier has retired it by then); pixels outside the image stay zero.  The (scale, shift) pairs
// of a channel block (512 B) arrive by one LDS-DMA piece with the patch.  The LDS reads / writes of this pass are
// inline asm: a compiler-visible LDS access behind an LDS-DMA gets an s_waitcnt vmcnt(0) (profiles/r02_gemm_debug.md).
// WS = weight slices in flight (LDS slots): 2 = the slice of the next tap is requested while this tap computes (vmcnt(0) per tap);
// 3 = two taps ahead with a counted wait (experiment, tile 103: ONE 16-wave workgroup per CU owning a 256-pixel patch).
template <int WM, int WN, int MI, int NI, int KG, bool GN, int WS = 2>
__global__ __launch_bounds__(WM * WN * KG * 64) void conv_halo_kernel(insv2v_gemm_desc p, int tw_shift) {
    constexpr int NWV = WM * WN * KG;
    constexpr int BM = WM * MI * 32, BN = WN * NI * 32;
    static_assert(BM == 128 || BM == 256, "the pixel patch is 128 (8x16 / 16x8) or 256 (16x16 / 32x8) output pixels");
    static_assert(WS == 2 || (WS == 3 && !GN && KG == 1), "the deep weight ring has no fused-GroupNorm / K-group form");
    constexpr int LD = BK;
    constexpr int RPP = 8 * NWV, RW = BN / RPP;
    constexpr int HPIECES = BM == 128 ? 23 : 43;      // 1 KiB DMA pieces (8 pixel rows each) covering <= 180 (<= 340) patch rows
    constexpr int HP = (HPIECES + NWV - 1) / NWV;     // pieces per wave
    constexpr int HALO_B = HPIECES * 1024;
    constexpr int KQ = BK / 16 / KG;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* sH = smem;                                  // [2][HALO_B] input patches (double buffered over channel blocks)
    half_t* sW = (half_t*)(smem + 2 * HALO_B);        // [WS][BN][LD] weight slices
    constexpr int RING_B = 2 * HALO_B + WS * BN * BK * 2, STAGE_B = BM * (BN + 4) * 4;
    float* sBias = (float*)(smem + (RING_B > STAGE_B ? RING_B : STAGE_B));
    constexpr int AB_OFF = (RING_B > STAGE_B ? RING_B : STAGE_B) + BN * 4;  // [2][64][2] floats (GN only)

    const int tid = threadIdx.x, lane = tid & 63;
#ifdef INSV2V_GEMM_PROF
    unsigned long long prof_t[6];
#endif
    PROF_MARK(0);
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kg = wid / (WM * WN), wl = wid % (WM * WN);
    // Round 3: N = 320 leaves the third 128-column tile half empty.  Waves are dealt to the SIMDs round robin (wid & 3), so the
    // column half of a wave is wl / WM, not wl % WN: the waves whose 64 columns lie beyond N then sit one per SIMD, skip their
    // fragment reads + MFMAs (they still issue their share of the DMA and keep the barriers), and every SIMD of the CU gets that
    // matrix-pipe / LDS time back for the other workgroup (bit 8 of tw_shift = the old mapping without the skip, for A/B).
    const bool legacy_map = (tw_shift >> 8) & 1;
    tw_shift &= 255;
    const int wm = legacy_map ? wl / WN : wl % WM, wn = legacy_map ? wl % WN : wl / WM;
    const int TW = 1 << tw_shift, TH = BM >> tw_shift;
    const int tiles_x = p.OW >> tw_shift, tiles_y = p.OH / TH, tiles_img = tiles_x * tiles_y;
    const int tiles_n = (p.N + BN - 1) / BN, tiles_m = p.NB * tiles_img;
    const int bid = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    constexpr int GROUP_M = 8;
    const int per_group = GROUP_M * tiles_n;
    const int gidx = bid / per_group, first_m = gidx * GROUP_M;
    const int gsz = min(GROUP_M, tiles_m - first_m), rin = bid - gidx * per_group;
    const int tn = rin / gsz, tm = first_m + rin - tn * gsz;
    const int bn0 = tn * BN;
    const int nb = tm / tiles_img, trem = tm - nb * tiles_img;
    const int ty = trem / tiles_x, tx = trem - ty * tiles_x;
    const int oy0 = ty * TH, ox0 = tx * TW;
    const int up = p.upsample ? 1 : 0;
    // source patch: rows sy0 .. sy0+PH-1, cols sx0 .. sx0+PW-1 (may stick out of the image: zero padding)
    const int sy0 = (oy0 - 1) >> up, sx0 = (ox0 - 1) >> up;
    const int PH = (TH >> up) + 2, PW = (TW >> up) + 2, HROWS = PH * PW;

    const half_t* A = (const half_t*)p.a;
    const half_t* A2 = p.a2 ? (const half_t*)p.a2 : A;
    const srd_t rA = make_srd(A), rA2 = make_srd(A2), rW = make_srd(p.w);

    // LDS swizzle of the patch: the 16-byte chunk index of pixel (hy, hx) is XORed with a key chosen so that the 16 lanes
    // of every ds_read_b128 group land on 16 distinct bank slots.  A group holds fragment rows {0-3, 12-15, 20-27} (or
    // {4-11, 16-19, 28-31}); in an 8x16 patch these are 16 different hx (mod 16) spread over two patch rows -> key from hx
    // alone; in a 16x8 patch they are 4 patch rows x 4 pixels -> the row parity supplies the fourth bit.  PW is even, so the
    // 128-byte half of the 256-byte bank row is hx & 1.  (Keyed on the linear row index the reads were 24-39 % conflicts.)
    auto patch_key = [&](int hy, int hx) { return ((hx >> 1) + (tw_shift == 3 ? ((hy & 1) << 2) : 0)) & 7; };
    // patch staging map: piece q = i*NWV + wid holds patch rows q*8 .. q*8+7 (row = pixel, 128 B = one channel block)
    unsigned hoff1[HP], hoff2[HP];
    int hchunk[HP];  // GN: logical 8-channel chunk of this lane's 16 bytes of piece i, or -1 for zero padding
#pragma unroll
    for (int i = 0; i < HP; ++i) {
        const int r = (i * NWV + wid) * 8 + (lane >> 3);
        const int hy = r / PW, hx = r - hy * PW;
        const int chunk = (lane & 7) ^ patch_key(hy, hx);
        const int iy = sy0 + hy, ix = sx0 + hx;
        const bool ok = r < HROWS && (unsigned)iy < (unsigned)p.IH && (unsigned)ix < (unsigned)p.IW;
        const int64_t pix = ((int64_t)nb * p.IH + iy) * p.IW + ix;
        hoff1[i] = ok ? (unsigned)((pix * p.lda + chunk * 8) * 2) : OOB_OFFSET;
        hoff2[i] = ok ? (unsigned)((pix * p.lda2 + chunk * 8) * 2) : OOB_OFFSET;
        hchunk[i] = ok ? chunk : -1;
    }
    const int crow = wid * 8 + (lane >> 3), cslot = lane & 7;
    unsigned woff[RW];
#pragma unroll
    for (int i = 0; i < RW; ++i) {
        const int row = crow + RPP * i;
        const int n = bn0 + row;
        woff[i] = n < p.N ? (unsigned)(((int64_t)n * p.ldw + (cslot ^ ((row >> 1) & 7)) * 8) * 2) : OOB_OFFSET;
    }
    const int ncb = p.Cin / BK, nk = ncb * 9;

    auto issue_halo = [&](int i, int cb) {  // piece i of this wave, channel block cb -> patch buffer cb & 1
        const int q = i * NWV + wid;
        if (q >= HPIECES) return;
        const int ci0 = cb * BK;
        const bool second = p.k_split > 0 && ci0 >= p.k_split;
        dma16(second ? rA2 : rA, second ? hoff2[i] : hoff1[i], (second ? ci0 - p.k_split : ci0) * 2, sH + (cb & 1) * HALO_B + q * 1024);
    };
    // ---- fused GroupNorm (+SiLU) of the input patch
    const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
    const srd_t rAB = make_srd(GN ? (const void*)p.gn_ab : p.w);
    const int gn_sample = GN ? nb / p.gn_images_per_sample : 0;
    auto issue_ab = [&](int cb) {  // (scale, shift) of channel block cb: 64 x 2 floats = 512 B = half a DMA piece
        if (GN && wid == 0 && lane < 32)
            dma16(rAB, (unsigned)((((int64_t)gn_sample * p.Cin + cb * BK) * 2 + lane * 4) * 4), 0, smem + AB_OFF + (cb & 1) * 512);
    };
    auto normalize = [&](int i, int cb) {  // this lane's 16 bytes of piece i of patch buffer cb & 1
        const int q = i * NWV + wid;
        if (!GN || q >= HPIECES) return;
        const unsigned addr = lds0 + (cb & 1) * HALO_B + q * 1024 + lane * 16;
        const unsigned abaddr = lds0 + AB_OFF + (cb & 1) * 512 + (hchunk[i] < 0 ? 0 : hchunk[i]) * 64;
        uint4r v;
        floatx4 c0, c1, c2, c3;
        asm volatile("ds_read_b128 %0, %5\n\tds_read_b128 %1, %6\n\tds_read_b128 %2, %6 offset:16\n\t"
                     "ds_read_b128 %3, %6 offset:32\n\tds_read_b128 %4, %6 offset:48\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(v), "=&v"(c0), "=&v"(c1), "=&v"(c2), "=&v"(c3) : "v"(addr), "v"(abaddr) : "memory");
        const half8 x = __builtin_bit_cast(half8, v);
        const float sc[8] = {c0[0], c0[2], c1[0], c1[2], c2[0], c2[2], c3[0], c3[2]};
        const float sh[8] = {c0[1], c0[3], c1[1], c1[3], c2[1], c2[3], c3[1], c3[3]};
        half8 y;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float t = fmaf((float)x[e], sc[e], sh[e]);
            if (p.gn_silu) t = silu_f(t);
            y[e] = hchunk[i] < 0 ? (half_t)0.f : (half_t)t;
        }
        const uint4r o = __builtin_bit_cast(uint4r, y);
        asm volatile("ds_write_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" ::"v"(addr), "v"(o) : "memory");
    };
    auto issue_w = [&](int buf, int cb, int tap) {
        char* w = (char*)(sW + buf * BN * LD) + wid * 1024;
        const int soff = (tap * p.Cin + cb * BK) * 2;
#pragma unroll
        for (int i = 0; i < RW; ++i) dma16(rW, woff[i], soff, w + i * (NWV * 1024));
    };

    floatx16 acc[NI][MI];
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < MI; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int frow = lane & 31, fhalf = lane >> 5;
    int fpy[MI], fpx[MI];  // output pixel (within the patch) of this lane's activation fragment rows
#pragma unroll
    for (int j = 0; j < MI; ++j) {
        const int ml = wm * MI * 32 + j * 32 + frow;
        fpy[j] = ml >> tw_shift;
        fpx[j] = ml & (TW - 1);
    }
    const int wsw = (frow >> 1) & 7;
    const bool wave_live = legacy_map || bn0 + wn * NI * 32 < p.N;   // wave-uniform
    auto compute = [&](int wbuf, int cb, int kh, int kw) {
        if (!wave_live) return;
        const half_t* hb = (const half_t*)(sH + (cb & 1) * HALO_B);
        const half_t* w = sW + wbuf * BN * LD + (wn * NI * 32 + frow) * LD;
        int arow[MI], akey[MI];
#pragma unroll
        for (int j = 0; j < MI; ++j) {
            const int uy = oy0 + fpy[j] + kh - 1, ux = ox0 + fpx[j] + kw - 1;  // tap position in (upsampled) image coords
            const int hy = (uy >> up) - sy0, hx = (ux >> up) - sx0;
            arow[j] = hy * PW + hx;
            akey[j] = patch_key(hy, hx);
        }
#pragma unroll
        for (int kq = 0; kq < KQ; ++kq) {
            const int kk = kg * KQ + kq;
            const int cl = kk * 2 + fhalf;
            half8 fa[MI], fw[NI];
#pragma unroll
            for (int j = 0; j < MI; ++j) fa[j] = *(const half8*)(hb + arow[j] * LD + ((cl ^ akey[j]) * 8));
#pragma unroll
            for (int i = 0; i < NI; ++i) fw[i] = *(const half8*)(w + i * 32 * LD + ((cl ^ wsw) * 8));
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < MI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fw[i], fa[j], acc[i][j], 0, 0, 0);
        }
    };

    float pre_b = 0.f;
    if (tid < BN && bn0 + tid < p.N && p.bias) pre_b = p.bias[bn0 + tid];
    issue_ab(0);
#pragma unroll
    for (int i = 0; i < HP; ++i) issue_halo(i, 0);
    issue_w(0, 0, 0);
    int cbn = 0, tapn = 1;   // WS = 3: (channel block, tap) of the next weight slice to request
    if (WS == 3) {
        if (tapn == 9) { tapn = 0; ++cbn; }
        if (nk > 1) issue_w(1, cbn, tapn);
        if (++tapn == 9) { tapn = 0; ++cbn; }
    }
    if (tid < BN) sBias[tid] = pre_b;
    if (GN) {  // the first patch is normalised before its first tap
        wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();   // the (scale, shift) piece of wave 0 has landed for everyone
#pragma unroll
        for (int i = 0; i < HP; ++i) normalize(i, 0);
    }
    int cb = 0, kh = 0, kw = 0, tap = 0;
    int wslot = 0, islot = 2;   // WS = 3: ring slot computed from / requested into
    for (int s = 0; s < nk; ++s) {
        // WS = 3: the last request of every step is the weight slice two taps ahead (patch pieces are requested BEFORE it), and a wave's
        // memory operations retire in issue order: all but the newest RW pieces landed = this tap's slice and every patch piece are in LDS
        if (WS == 3 && s + 1 < nk) wait_vmcnt<RW>();
        else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#ifdef INSV2V_GEMM_PROF
        if (s == 0) PROF_MARK(1);
#endif
        // GN: the piece requested one tap ago has landed (wait above) -> normalise it before this tap's DMA is issued
        if (GN && cb + 1 < ncb) {
#pragma unroll
            for (int i = 0; i < HP; ++i)  // static piece index: a runtime index would put hchunk[] in scratch
                if (tap == i + 1) normalize(i, cb + 1);
        }
        if (WS == 2 && s + 1 < nk) {
            const bool wrap = tap == 8;
            issue_w((s + 1) & 1, wrap ? cb + 1 : cb, wrap ? 0 : tap + 1);
        }
        if (tap == 0 && cb + 1 < ncb) issue_ab(cb + 1);
        if (cb + 1 < ncb) {  // the next block's patch trickles in, one piece per tap (static piece index: no scratch)
#pragma unroll
            for (int i = 0; i < HP; ++i)
                if (tap == i) issue_halo(i, cb + 1);
        }
        if (WS == 3) {
            if (s + 2 < nk) {
                issue_w(islot, cbn, tapn);
                if (++tapn == 9) { tapn = 0; ++cbn; }
            }
            islot = islot == 2 ? 0 : islot + 1;
        }
        compute(WS == 3 ? wslot : (s & 1), cb, kh, kw);
        if (WS == 3) wslot = wslot == 2 ? 0 : wslot + 1;
        if (++kw == 3) { kw = 0; ++kh; }
        if (++tap == 9) { tap = 0; kh = 0; ++cb; }
    }
    wait_vmcnt<0>();
    __syncthreads();
    PROF_MARK(2);
    tile_epilogue<WM, WN, MI, NI, KG, false>(p, acc, smem, sBias, nullptr, nullptr, tid, wm, wn, kg, bn0, 0, 0, true,
                                             [&](int r) { return (nb * p.OH + oy0 + (r >> tw_shift)) * p.OW + ox0 + (r & (TW - 1)); }
#ifdef INSV2V_GEMM_PROF
                                             , prof_t
#endif
    );
}

template <int WM, int WN, int MI, int NI, int KG, bool GN = false, int WS = 2>
static int launch_halo(const insv2v_gemm_desc& d, int tw_shift, hipStream_t s) {
    constexpr int BM = WM * MI * 32, BN = WN * NI * 32;
    constexpr size_t ring = 2 * (BM == 128 ? 23 : 43) * 1024 + WS * (size_t)BN * BK * sizeof(half_t);
    constexpr size_t stage = (size_t)BM * (BN + 4) * sizeof(float);
    constexpr size_t lds = (ring > stage ? ring : stage) + (size_t)BN * sizeof(float) + (GN ? 1024 : 0);
    static bool attr_set = false;
    if (const int e = set_dynamic_lds(attr_set, (const void*)conv_halo_kernel<WM, WN, MI, NI, KG, GN, WS>, lds)) return e;
    const int tiles = d.NB * (d.OH * d.OW / BM) * ((d.N + BN - 1) / BN);
    hipLaunchKernelGGL((conv_halo_kernel<WM, WN, MI, NI, KG, GN, WS>), dim3(tiles), dim3(WM * WN * KG * 64), lds, s, d, tw_shift);
    return launch_status();
}

template <int WM, int WN, int MI, int NI, int MODE, int STAGES, int KG = 1>
static int launch_cfg(const insv2v_gemm_desc& d, hipStream_t s) {
    constexpr int BM = WM * MI * 32, BN = WN * NI * 32;
    constexpr size_t lds = tile_lds_bytes(BM, BN, STAGES);
    if (lds > TILE_LDS_MAX) return INSV2V_EUNSUPPORTED;   // (plan_gemm refuses such a tile code first)
    static bool attr_set = false;
    if (const int e = set_dynamic_lds(attr_set, (const void*)gemm_kernel<WM, WN, MI, NI, MODE, STAGES, KG>, lds)) return e;
    int tiles = ((d.M + BM - 1) / BM) * ((d.N + BN - 1) / BN);
    dim3 grid(tiles, d.batch > 0 ? d.batch : 1, d.split_k > 1 ? d.split_k : 1);
    hipLaunchKernelGGL((gemm_kernel<WM, WN, MI, NI, MODE, STAGES, KG>), grid, dim3(WM * WN * KG * 64), lds, s, d);
    return launch_status();
}

// tile shapes: gemm_plan.h (tile_bm / tile_bn restate the sizes these template arguments give)
template <int MODE, int STAGES>
static int dispatch_tile(const insv2v_gemm_desc& d, int tile, hipStream_t s) {
    switch (tile) {
        case 1: return launch_cfg<2, 2, 2, 2, MODE, STAGES>(d, s);
        case 2: return launch_cfg<2, 2, 1, 2, MODE, STAGES>(d, s);
        case 3: return launch_cfg<2, 2, 2, 1, MODE, STAGES>(d, s);
        case 4: return launch_cfg<2, 2, 1, 1, MODE, STAGES>(d, s);
        case 5: return launch_cfg<4, 2, 1, 2, MODE, STAGES>(d, s);
        case 6: return launch_cfg<4, 2, 2, 2, MODE, STAGES>(d, s);
        case 7: return launch_cfg<4, 2, 1, 1, MODE, STAGES>(d, s);
        case 8: return launch_cfg<2, 2, 2, 2, MODE, STAGES, 2>(d, s);  // 128x128, 2 K groups of 4 waves
        case 9: return launch_cfg<2, 2, 2, 1, MODE, STAGES, 2>(d, s);  // 128x64,  2 K groups of 4 waves
    }
    return INSV2V_EINVAL;
}

// Split-K second pass: out = epilogue(sum_s partial[s]) with the same epilogue semantics as the main
// kernel (alpha, bias, row bias, SiLU, residual; fp16 or fp32 store).  8 outputs per thread.
__global__ __launch_bounds__(256) void splitk_reduce_kernel(insv2v_gemm_desc p, const float* ws, int nsplit) {
    const int64_t nchunk = (int64_t)p.M * (p.N / 8);
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nchunk) return;
    const int m = (int)(idx / (p.N / 8)), n = (int)(idx - (int64_t)m * (p.N / 8)) * 8;
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* src = ws + (int64_t)m * p.N + n;
    const int64_t slab = (int64_t)p.M * p.N;
    // everything this thread needs is requested up front (16-byte loads): residual, bias, row bias, then the slabs four at a time
    const bool res_vec = p.residual && (p.ldr & 7) == 0 && (((uintptr_t)p.residual & 15) == 0);
    half8 rh = {0, 0, 0, 0, 0, 0, 0, 0};
    if (res_vec) rh = *(const half8*)((const half_t*)p.residual + (int64_t)m * p.ldr + n);
    float4 b0 = make_float4(0.f, 0.f, 0.f, 0.f), b1 = b0, r0 = b0, r1 = b0;
    if (p.bias) {
        if (((uintptr_t)p.bias & 15) == 0) { b0 = *(const float4*)(p.bias + n); b1 = *(const float4*)(p.bias + n + 4); }
        else { b0 = make_float4(p.bias[n], p.bias[n + 1], p.bias[n + 2], p.bias[n + 3]); b1 = make_float4(p.bias[n + 4], p.bias[n + 5], p.bias[n + 6], p.bias[n + 7]); }
    }
    if (p.row_bias) {
        const float* rb = p.row_bias + (int64_t)(m / p.rows_per_group) * p.ld_rb + n;
        if ((p.ld_rb & 3) == 0 && (((uintptr_t)p.row_bias & 15) == 0)) { r0 = *(const float4*)rb; r1 = *(const float4*)(rb + 4); }
        else { r0 = make_float4(rb[0], rb[1], rb[2], rb[3]); r1 = make_float4(rb[4], rb[5], rb[6], rb[7]); }
    }
    int s = 0;
    for (; s + 4 <= nsplit; s += 4) {
        float4 a[4], b[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { a[u] = *(const float4*)(src + (s + u) * slab); b[u] = *(const float4*)(src + (s + u) * slab + 4); }
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // fixed summation order s = 0, 1, 2, ...: deterministic
            v[0] += a[u].x; v[1] += a[u].y; v[2] += a[u].z; v[3] += a[u].w; v[4] += b[u].x; v[5] += b[u].y; v[6] += b[u].z; v[7] += b[u].w;
        }
    }
    for (; s < nsplit; ++s) {
        const float4 a = *(const float4*)(src + s * slab), b = *(const float4*)(src + s * slab + 4);
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
    }
    const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w}, rr[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        float x = v[e] * p.alpha;
        if (p.bias) x += bb[e];
        if (p.row_bias) x += rr[e];
        if (p.act == INSV2V_ACT_SILU) x = silu_f(x);
        else if (p.act == INSV2V_ACT_QUICK_GELU) x = quick_gelu_f(x);
        else if (p.act >= INSV2V_ACT_RELU) x = act_raft_f(x, p.act);
        if (p.residual) x += res_vec ? (float)rh[e] : (float)((const half_t*)p.residual)[(int64_t)m * p.ldr + n + e];
        v[e] = x;
    }
    if (p.c_fp32) {
        float* dst = (float*)p.c + (int64_t)m * p.ldc + n;
#pragma unroll
        for (int e = 0; e < 8; ++e) dst[e] = v[e];
    } else {
        half_t* dst = (half_t*)p.c + (int64_t)m * p.ldc + n;
        if ((p.ldc & 7) == 0 && (((uintptr_t)p.c & 15) == 0)) {
            half8 h;
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = (half_t)v[e];
            *(half8*)dst = h;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) dst[e] = (half_t)v[e];
        }
    }
}

// (mean, rstd) pairs from the producer's partial sums, for the kernels that park finished statistics (gemm_q8 / gemm_r8 / gemm_w4)
__global__ __launch_bounds__(256) void ln_finalize_kernel(const float2* parts, float2* stats, int M, int nparts, int C, float eps) {
    const int m = blockIdx.x * 256 + threadIdx.x;
    if (m >= M) return;
    float s1 = 0.f, s2 = 0.f;
    for (int j = 0; j < nparts; ++j) { const float2 t = parts[(int64_t)j * M + m]; s1 += t.x; s2 += t.y; }
    const float mean = s1 / C;
    stats[m] = make_float2(mean, rsqrtf(fmaxf(s2 / C - mean * mean, 0.f) + eps));
}

// The A/B switches of the GEMM path (gemm_plan.h), read from the environment once for the library.
const gemm_switches& insv2v_gemm_switches() {
    static const gemm_switches sw = [] {
        auto env = [](const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; };
        gemm_switches s;
        s.r8 = env("INSV2V_GEMM_R8", s.r8); s.r8_stats = env("INSV2V_R8_STATS", s.r8_stats); s.q8_min_n = env("INSV2V_Q8_MIN_N", s.q8_min_n); s.persistent = env("INSV2V_GEMM_PERSISTENT", s.persistent);
        s.r8_geglu = env("INSV2V_R8_GEGLU", s.r8_geglu); s.r8_cim = env("INSV2V_R8_CIM", s.r8_cim); s.halo_legacy_map = env("INSV2V_HALO_LEGACY_MAP", s.halo_legacy_map);
        s.r8_dephase = env("INSV2V_R8_DEPHASE", s.r8_dephase); s.w4_wgs = env("INSV2V_W4_WGS", s.w4_wgs); s.w4_delay = env("INSV2V_W4_DELAY", s.w4_delay);
        return s;
    }();
    return sw;
}

// Bytes of one operand window of insv2v_gemm (0 = the hardware's: 2 GiB less a margin).  Tests shrink it so that small problems take the
// split path (insv2v_set_operand_window); the product never touches it.
static int64_t g_operand_window = 0;
extern "C" int64_t insv2v_set_operand_window(int64_t bytes) {
    const int64_t prev = g_operand_window;
    g_operand_window = bytes > 0 ? bytes : 0;
    return prev;
}
static int64_t operand_window() { return g_operand_window > 0 ? g_operand_window : ((int64_t)1 << 31) - ((int64_t)1 << 20); }
int64_t insv2v_operand_window_override() { return g_operand_window; }   // (the row launchers split by the same hook: rows_common.h)

// ONE planner (gemm_plan.h) answers for the launch and for the three read-only entries, so that they cannot disagree
static insv2v_gemm_plan_t plan_here(const insv2v_gemm_desc& d, int cus = 0, bool queries_only = false) {
    return plan_gemm(d, cus > 0 ? cus : insv2v_num_cus(), operand_window(), insv2v_gemm_switches(), queries_only);
}
extern "C" int insv2v_gemm_plan(const insv2v_gemm_desc* dp, int cus, insv2v_gemm_plan_t* out) {
    if (!dp || !out) return INSV2V_EINVAL;
    *out = plan_here(*dp, cus);
    return 0;
}
extern "C" int insv2v_gemm_stats_parts(const insv2v_gemm_desc* dp) {
    const int w = dp ? plan_here(*dp, 0, true).stats_width : 0;
    return w ? (dp->N + w - 1) / w : 0;
}
extern "C" int insv2v_conv3x3_fuses_groupnorm(const insv2v_gemm_desc* dp) { return dp ? plan_here(*dp, 0, true).gn_fuse : 0; }

// the persistent kernels park finished (mean, rstd) pairs: partial sums from a producer are finalised by a small launch first
static void finish_stats(insv2v_gemm_desc& d, hipStream_t s) {
    hipLaunchKernelGGL(ln_finalize_kernel, dim3((d.M + 255) / 256), dim3(256), 0, s, (const float2*)d.row_stats, (float2*)d.stats_scratch, d.M,
                       d.stats_parts, d.K, d.ln_eps);
    stats_finished(d);
}

// one in-window problem, as planned
static int execute(insv2v_gemm_desc d, const insv2v_gemm_plan_t& p, hipStream_t s) {
    if (p.ln_finalize) finish_stats(d, s);
    const insv2v_gemm_desc full = d;
    if (p.split_k > 1) splitk_main_pass(d, p.split_k);
    else d.split_k = 1;
    const bool conv = d.mode == INSV2V_MODE_CONV3X3;
    int rc = INSV2V_EINVAL;
    switch (p.family) {
        case INSV2V_PLAN_Q8: return insv2v_gemm_q8(d, p.variant, s);
        case INSV2V_PLAN_R8: return insv2v_gemm_r8(d, p.variant, s);
        case INSV2V_PLAN_W4: return insv2v_gemm_w4(d, p.variant, s);
        case INSV2V_PLAN_HALO:
            switch (p.variant) {
                case 0: return d.gn_ab ? launch_halo<4, 2, 1, 2, 1, true>(d, p.tw_shift, s) : launch_halo<4, 2, 1, 2, 1>(d, p.tw_shift, s);
                case 3: return launch_halo<8, 2, 1, 2, 1, false, 3>(d, p.tw_shift, s);  // ONE 16-wave workgroup per CU, for A/B measurement
                case 2: return launch_halo<2, 2, 2, 2, 1>(d, p.tw_shift, s);            // 4 waves with 64 x 64 wave tiles, for A/B measurement
                case 1: return launch_halo<2, 2, 2, 2, 2>(d, p.tw_shift, s);            // K-group variant, kept for A/B measurement
            }
            return rc;
        case INSV2V_PLAN_TILE:
            // (An L2 prefetch of slices 3 steps ahead was measured and removed: 30-45 % slower, profiles/README.md.)
            switch (p.ring) {
                case 2: rc = conv ? dispatch_tile<INSV2V_MODE_CONV3X3, 2>(d, p.variant, s) : dispatch_tile<INSV2V_MODE_LINEAR, 2>(d, p.variant, s); break;
                case 3: rc = conv ? dispatch_tile<INSV2V_MODE_CONV3X3, 3>(d, p.variant, s) : dispatch_tile<INSV2V_MODE_LINEAR, 3>(d, p.variant, s); break;
                case 4: rc = conv ? dispatch_tile<INSV2V_MODE_CONV3X3, 4>(d, p.variant, s) : dispatch_tile<INSV2V_MODE_LINEAR, 4>(d, p.variant, s); break;
            }
            if (rc != 0 || !p.splitk_reduce) return rc;
            hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)(((int64_t)full.M * (full.N / 8) + 255) / 256)), dim3(256), 0, s, full, (const float*)full.workspace, p.split_k);
            return launch_status();
    }
    return rc;
}

static int run(const insv2v_gemm_desc& d, hipStream_t s);
// a problem beyond the operand window: p.parts launches over row (LINEAR) / image (CONV3X3) ranges, each planned on its own
static int run_parts(insv2v_gemm_desc f, const insv2v_gemm_plan_t& p, hipStream_t s) {
    if (p.ln_finalize) finish_stats(f, s);
    const int64_t total = f.mode == INSV2V_MODE_CONV3X3 ? f.NB : f.M, per = p.units_per_part;
    for (int64_t u0 = 0; u0 < total; u0 += per)
        if (const int rc = run(window_part(f, u0, std::min(per, total - u0)), s)) return rc;
    return 0;
}
static int run(const insv2v_gemm_desc& d, hipStream_t s) {
    const insv2v_gemm_plan_t p = plan_here(d);
    return p.rc ? p.rc : p.parts > 1 ? run_parts(d, p, s) : execute(d, p, s);
}

extern "C" int insv2v_gemm(const insv2v_gemm_desc* dp, insv2v_stream_t stream) {
    if (!one_device() || !dp) return INSV2V_EINVAL;
    insv2v_gemm_desc d = *dp;
    gemm_defaults(d);
    return run(d, as_stream(stream));
}

#ifdef INSV2V_GEMM_PROF
extern "C" int insv2v_prof_read(unsigned long long* out, int reset) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_prof), sizeof(unsigned long long) * 8);
    if (e == hipSuccess && reset) {
        unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        e = hipMemcpyToSymbol(HIP_SYMBOL(g_prof), z, sizeof(z));
    }
    return (int)e;
}
#endif
