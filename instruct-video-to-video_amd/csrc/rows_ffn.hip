// Fused feed-forward (insv2v_ffn_fused) and the K = 320 / 640 row Linear (insv2v_rowlin); the register-resident scheme: rows_common.h
#include "rows_common.h"
#include "rows_plan.h"
#include <algorithm>
#include <cstdlib>

namespace {
constexpr int NCHUNK = 4 * FC / 32;     // 40 chunks of 32 hidden units
constexpr int CT = FC / 32;             // 10 output channel tiles
constexpr int W1_FR = 2 * (KS1 + 1);    // 42 fragments of a chunk's first contraction (also: of a pair of output tiles of a Linear)
constexpr int W2_FR = 2 * CT;           // 20 fragments of a chunk's second contraction

// ===================================================================================================== feed-forward
struct FfnArgs {
    const half_t* x;
    half_t* out;
    const half_t* wstream;
    const half_t* res2;    // POST: residual of the trailing Linear (the transformer module's input), row stride ldr2
    int64_t ldx, ldo, ldr2;
    int M;
    float eps;
};
// stream per pass, in 64-fragment sections: [b2: 10][W1(0): 42][pad 12] | stage k = 0..38: [W1(k+1): 42][W2(k): 20][pad 2] | [W2(39): 20][pad 12]
constexpr int FFN_SLOT_FR = 32, FFN_NS = 4;
constexpr int FFN_PASS_SLOTS = (64 + 64 * (NCHUNK - 1) + 32) / FFN_SLOT_FR;
// POST: the transformer module's trailing Linear (proj_out, attention.py:89 / motion_module.py:146) + its residual ride behind the feed-
// forward: out = Wp . (x + FF(LN(x))) + bp + res2.  The feed-forward result never leaves the registers: its accumulator tiles (+ x) packed
// to fp16 are the B fragments of the projection.  Stream: + [output tiles in pairs x 21 k-steps: 210][pad 14] = 7 more slots.
constexpr int FFN_POST_FR = 224, FFN_POST_SLOTS = FFN_POST_FR / FFN_SLOT_FR;
typedef unsigned uint2v __attribute__((__vector_size__(8)));   // (the 8-byte buffer-load builtin traffics in GCC-style vectors)

// (The timing ablations and schedule variants that shaped this kernel - no refills / no GEGLU / no barriers, GEGLU of a stage in one lump,
// S values pinned per pair, a five-slot ring - were template variants of it; their results: profiles/r03_ffn_fused_ablation.txt,
// profiles/r05_ffn_interleaved_geglu.txt.)
template <bool POST>
__global__ __launch_bounds__(256, 1) void ffn_fused_kernel(FfnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];   // the weight ring, nothing else
    typedef Ring<FFN_SLOT_FR, FFN_NS> R;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tok = lane & 31, half = lane >> 5;
    const int ntiles = (p.M + 127) / 128;
    const srd_t rX = make_srd(p.x);
    R ring;
    ring.init(smem, p.wstream, FFN_PASS_SLOTS + (POST ? FFN_POST_SLOTS : 0), wid, lane);

    const half8 ones = bias_ones(half);

#pragma unroll 1
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int m = tile * 128 + wid * 32 + tok;
        const bool mok = m < p.M;
        const unsigned xoff = mok ? (unsigned)(((int64_t)m * p.ldx + 8 * half) * 2) : OOB_OFFSET;
        half8 xf[KS1];
        load_rows<KS1, true>(xf, rX, xoff, p.eps);

        floatx16 O[CT];
        floatx16 Sh, Sg, Nh, Ng;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) zero16(O[ct]);
        zero16(Sh); zero16(Sg);
        half8 pf[2] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
        half8 fb[2][8];
        // what a fragment position means: kind 0 = prologue section, 1 = steady stage, 2 = final section.  (nh, ng) = the S being accumulated
        auto consume_group = [&](auto kind_, auto g_, floatx16& nh, floatx16& ng) {
            constexpr int kind = decltype(kind_)::value, g = decltype(g_)::value;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int f = g * 8 + i;
                const half8 a = fb[g & 1][i];
                if (kind == 0) {                    // [b2: 10] [W1(0): 42] [pad]
                    if (f < CT) O[f < CT ? f : 0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, ones, O[f < CT ? f : 0], 0, 0, 0);
                    else if (f < CT + W1_FR) {
                        const int w = f - CT, s = w >> 1;
                        const half8 b = s < KS1 ? xf[s < KS1 ? s : 0] : ones;
                        if (w & 1) ng = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, ng, 0, 0, 0);
                        else nh = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, nh, 0, 0, 0);
                    }
                } else if (kind == 1) {             // [W1(k+1): 42] [W2(k): 20] [pad 2]
                    if (f < W1_FR) {
                        const int s = f >> 1;
                        const half8 b = s < KS1 ? xf[s < KS1 ? s : 0] : ones;
                        if (f & 1) ng = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, ng, 0, 0, 0);
                        else nh = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, nh, 0, 0, 0);
                    } else if (f < W1_FR + W2_FR) {
                        const int j = f - W1_FR, s2 = j / CT, ct = j - s2 * CT;
                        O[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pf[s2], O[ct], 0, 0, 0);
                    }
                } else {                            // [W2(39): 20] [pad 12]
                    if (f < W2_FR) {
                        const int s2 = f / CT, ct = f - s2 * CT;
                        O[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pf[s2], O[ct], 0, 0, 0);
                    }
                }
                if (i == 3) ring.template refill<g % R::GPS, 0>();
                if (i == 7) ring.template refill<g % R::GPS, 1>();
            }
        };
#define RD(g) ring.template read_group<g>(fb[(g) & 1])
#define CG(kind, g, nh, ng) consume_group(ic<kind>{}, ic<g>{}, nh, ng)

        // ---- prologue section: O = b2, S(0) = W1(0) . x + b1
        RD(0);
        RD(1); CG(0, 0, Sh, Sg);
        RD(2); CG(0, 1, Sh, Sg);
        RD(3); CG(0, 2, Sh, Sg);
        RD(4); CG(0, 3, Sh, Sg);
        RD(5); CG(0, 4, Sh, Sg);
        RD(6); CG(0, 5, Sh, Sg);
        RD(7); CG(0, 6, Sh, Sg);
        // (group 7 of the prologue is padding: zeros; the first stage "consumes" it against P = 0)

        // ---- steady state: stage k = S(k+1), then O += W2(k) . P(k); the tail of W2(k) is consumed at the start of stage k+1
        // GEGLU(k) = 8 pairs of hidden units, ONE pair per fragment group, spread between that group's MFMAs by the scheduler pipeline
        // below (~3 VALU per MFMA; the lump this replaces sat between two MFMAs with the matrix pipe idle: ~190 VALU, a quarter of
        // the kernel).  S(k) is complete behind the 2nd MFMA of stage k-1's group 5, so its pairs 0, 1 ride in groups 5, 6 of stage
        // k-1 and pairs 2 .. 7 in groups 7, 0 .. 4 of stage k; W2(k) starts in group 5.  P(k-1) is still read by stage k's group 7
        // (tail of W2(k-1)): two P buffers, and the two S sets, swap roles from stage to stage (no copies).
        uint4v PA[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}}, PB[2] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        auto gpair = [&](auto pr_, const floatx16& sh, const floatx16& sg, uint4v (&P)[2]) {
            constexpr int pr = decltype(pr_)::value, e0 = pr < 4 ? 2 * pr : 8 + 2 * (pr - 4);
            const float h0 = sh[e0], h1 = sh[e0 + 1], g0 = sg[e0], g1 = sg[e0 + 1];
            P[pr >> 2][pr & 3] = pk2(h0 * gelu_erf_relu_f(g0), h1 * gelu_erf_relu_f(g1));
        };
        // group g of a steady stage: MFMAs of W1(k+1) into (nh, ng) / of W2 against Pw; pair pr of the GEGLU of (sh, sg) into Pg
        auto cgi = [&](auto g_, auto pr_, const floatx16& sh, const floatx16& sg, floatx16& nh, floatx16& ng, uint4v (&Pw)[2], uint4v (&Pg)[2]) {
            constexpr int g = decltype(g_)::value;
            // the eight fragments of this group were read one group ago, behind them only the eight reads just issued
            __builtin_amdgcn_s_waitcnt(0xC87F);   // lgkmcnt(8), nothing else
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int f = g * 8 + i;
                const half8 a = fb[g & 1][i];
                if (f < W1_FR) {
                    const int s = f >> 1;
                    const half8 b = s < KS1 ? xf[s < KS1 ? s : 0] : ones;
                    if (f & 1) ng = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, ng, 0, 0, 0);
                    else nh = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, nh, 0, 0, 0);
                } else if (f < W1_FR + W2_FR) {
                    const int j = f - W1_FR, s2 = j / CT, ct = j - s2 * CT;
                    O[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, __builtin_bit_cast(half8, Pw[s2]), O[ct], 0, 0, 0);
                }
                if (i == 3) ring.template refill<g % R::GPS, 0>();
                if (i == 7) ring.template refill<g % R::GPS, 1>();
            }
            // (behind the MFMAs in program order: group 5's first two complete the S its pair reads; the pipeline below places it)
            gpair(pr_, sh, sg, Pg);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
            }
        };
        // (sh, sg) = S(k), (nh, ng) <- S(k+1), Pc = P(k), Pn = P(k-1) until group 7 is through, then P(k+1)
        auto stage = [&](floatx16& sh, floatx16& sg, floatx16& nh, floatx16& ng, uint4v (&Pc)[2], uint4v (&Pn)[2]) {
            RD(0); cgi(ic<7>{}, ic<2>{}, sh, sg, nh, ng, Pn, Pc);
            zero16(nh); zero16(ng);
            RD(1); cgi(ic<0>{}, ic<3>{}, sh, sg, nh, ng, Pc, Pc);
            RD(2); cgi(ic<1>{}, ic<4>{}, sh, sg, nh, ng, Pc, Pc);
            RD(3); cgi(ic<2>{}, ic<5>{}, sh, sg, nh, ng, Pc, Pc);
            RD(4); cgi(ic<3>{}, ic<6>{}, sh, sg, nh, ng, Pc, Pc);
            RD(5); cgi(ic<4>{}, ic<7>{}, sh, sg, nh, ng, Pc, Pc);
            RD(6); cgi(ic<5>{}, ic<0>{}, nh, ng, nh, ng, Pc, Pn);
            RD(7); cgi(ic<6>{}, ic<1>{}, nh, ng, nh, ng, Pc, Pn);
        };
        gpair(ic<0>{}, Sh, Sg, PA); gpair(ic<1>{}, Sh, Sg, PA);
        static_assert((NCHUNK - 1) % 2 == 1, "steady stages: pairs + one");
#pragma unroll 1
        for (int k = 0; k < (NCHUNK - 1) / 2; ++k) { stage(Sh, Sg, Nh, Ng, PA, PB); stage(Nh, Ng, Sh, Sg, PB, PA); }
        stage(Sh, Sg, Nh, Ng, PA, PB);
        // ---- final section: tail of W2(38) against P(38) = PA, the rest of GEGLU(39), W2(39) against PB
        pf[0] = __builtin_bit_cast(half8, PA[0]); pf[1] = __builtin_bit_cast(half8, PA[1]);
        RD(0); CG(1, 7, Sh, Sg);
        gpair(ic<2>{}, Nh, Ng, PB); gpair(ic<3>{}, Nh, Ng, PB); gpair(ic<4>{}, Nh, Ng, PB);
        gpair(ic<5>{}, Nh, Ng, PB); gpair(ic<6>{}, Nh, Ng, PB); gpair(ic<7>{}, Nh, Ng, PB);
        pf[0] = __builtin_bit_cast(half8, PB[0]); pf[1] = __builtin_bit_cast(half8, PB[1]);
        RD(1); CG(2, 0, Nh, Ng);
        RD(2); CG(2, 1, Nh, Ng);
        CG(2, 2, Nh, Ng);
        ring.template refill<3 % R::GPS, 0>(); ring.template refill<3 % R::GPS, 1>();
#undef CG
#undef RD

        const srd_t rO = make_srd(p.out);
        const unsigned ooff = mok ? (unsigned)(((int64_t)m * p.ldo + 8 * half) * 2) : OOB_OFFSET;
        if constexpr (!POST) {
            // ---- epilogue: out = O + x (raw, re-read: L2-hot)
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                uint4v rv[2];
                load_res_tile<true>(rv, rX, xoff, ct * 64);
                store_tile<true>(O[ct], rv, rO, ooff, ct * 64);
            }
        } else {
            // ---- h = O + x in the C layout (8-byte residual pieces: channels 32 ct + 8 q + 4 half .. +3), packed: the B fragments of the
            // trailing projection (k-steps 2 ct, 2 ct + 1), into the registers that held the normalised x
            const unsigned xoff4 = mok ? (unsigned)(((int64_t)m * p.ldx + 4 * half) * 2) : OOB_OFFSET;
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) {
                uint2v res[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) res[q] = __builtin_amdgcn_raw_buffer_load_b64(rX, xoff4, (ct * 32 + q * 8) * 2, 0);
                floatx16 hsum;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const unsigned rlo = res[q][0], rhi = res[q][1];   // (scalars first: bit_cast on a vector subscript takes element 0)
                    const half2v r0 = __builtin_bit_cast(half2v, rlo), r1 = __builtin_bit_cast(half2v, rhi);
                    hsum[4 * q] = O[ct][4 * q] + (float)r0[0]; hsum[4 * q + 1] = O[ct][4 * q + 1] + (float)r0[1];
                    hsum[4 * q + 2] = O[ct][4 * q + 2] + (float)r1[0]; hsum[4 * q + 3] = O[ct][4 * q + 3] + (float)r1[1];
                }
                pack_tile(hsum, xf[2 * ct], xf[2 * ct + 1]);
            }
            // ---- out = Wp . h + bp + res2: output tiles in pairs (two MFMA chains), fragment f of the section = (k-step (f % 42) >> 1, tile
            // 2 (f / 42) + (f & 1)); the pipeline restarts here (one fragment-read latency per row tile)
            const srd_t rR2 = make_srd(p.res2);
            const unsigned roff2 = mok ? (unsigned)(((int64_t)m * p.ldr2 + 8 * half) * 2) : OOB_OFFSET;
            floatx16 acc0, acc1;
            uint4v resv[2][2];
            auto consume_post = [&](auto g_) {
                constexpr int g = decltype(g_)::value;
                static_for<8>([&](auto i_) {
                    constexpr int i = decltype(i_)::value, f = g * 8 + i;
                    if constexpr (f < 5 * W1_FR) {
                        constexpr int pr = f / W1_FR, s = (f % W1_FR) >> 1;
                        const half8 b = s < KS1 ? xf[s < KS1 ? s : 0] : ones;
                        if constexpr ((f & 1) == 0) {
                            if constexpr (s == 0) { zero16(acc0); load_res_tile<true>(resv[0], rR2, roff2, pr * 128); load_res_tile<true>(resv[1], rR2, roff2, pr * 128 + 64); }
                            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[g & 1][i], b, acc0, 0, 0, 0);
                        } else {
                            if constexpr (s == 0) zero16(acc1);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[g & 1][i], b, acc1, 0, 0, 0);
                            if constexpr (s == KS1) {
                                store_tile<true>(acc0, resv[0], rO, ooff, pr * 128);
                                store_tile<true>(acc1, resv[1], rO, ooff, pr * 128 + 64);
                            }
                        }
                    }
                    if (i == 3) ring.template refill<g % R::GPS, 0>();
                    if (i == 7) ring.template refill<g % R::GPS, 1>();
                });
            };
            constexpr int NGP = FFN_POST_FR / 8;
            ring.template read_group<0>(fb[0]);
            static_for<NGP - 1>([&](auto g_) {
                constexpr int g = decltype(g_)::value;
                ring.template read_group<g + 1>(fb[(g + 1) & 1]);
                consume_post(ic<g>{});
            });
            consume_post(ic<NGP - 1>{});
        }
    }
    wait_vmcnt<0>();   // no LDS-DMA may land after this workgroup's LDS has been handed to another one
}

// ===================================================================================================== Linear, K = 320
struct RowLinArgs {
    const half_t* x;
    half_t* out;
    const half_t* residual;
    const half_t* wstream;
    int64_t ldx, ldo, ldr;
    int M, N;
    int rows_per_frame, frames;   // FRAME: bias row = (m / rows_per_frame) % frames (<= 16)
    float eps;
    float* stats;                 // optional [M][2] (mean, rstd) of the OUTPUT rows, for the LayerNorm that follows
    float stats_eps;
    const float* gn_ab;           // GN: [samples][K][2] (scale, shift) of a preceding GroupNorm; sample = m / gn_rows
    int gn_rows;
    int gn_units, gn_tiles;       // GN: 32-row wave blocks per sample = ceil(gn_rows / 32); 128-row tiles of the segmented schedule (insv2v_rowlin)
};
// stream per pass: per PAIR of 32-row output tiles (2p, 2p+1) one section of GP groups of 8 fragments (a whole number of 16-fragment slots):
//   [for k-step s = 0..KS: (tile 2p, tile 2p+1)] = 2 (KS + 1) fragments, then padding;  s = KS is the bias step
//   K = 320: 42 fragments in 6 groups (3 slots); K = 640: 82 fragments in 12 groups (6 slots)
constexpr int LIN_SLOT_FR = 16;
template <int KS> struct LinCfg {
    static constexpr int FR = 2 * (KS + 1);                  // fragments of a pair
    static constexpr int GP = (FR + 15) / 16 * 2;            // groups per pair section
    // K = 320: 160-250 registers suffice, so TWO workgroups share a CU (64 KiB ring each): one wave's MFMAs cover the other's fragment
    // reads, waits and ring bookkeeping - the overlap a lone wave per SIMD cannot have.  K = 640 holds 160 registers of activations:
    // one workgroup per CU with the deep ring.
    static constexpr int WGS = KS <= 20 ? 2 : 1;
    static constexpr int NS = KS <= 20 ? 4 : 9;
    // K = 640, TB = 2 (template parameter of the kernel): a wave owns TWO 32-token blocks (256 rows per workgroup), so every weight fragment
    // read from LDS feeds two MFMAs - one MFMA per fragment keeps the LDS port as busy as the matrix pipe (1 KiB per 32 cycles per SIMD)
    // and capped the kernel at ~33 % matrix utilisation; 320 activation + 64 accumulator + 64 fragment registers of the 512 a lone wave
    // per SIMD may use (the forms that also hold residual tiles spill 8-142 registers outside the pair loop and still win at 10 stacked
    // clips: +3-8 % per launch; the GroupNorm form stays at TB = 1).
};

// GroupNorm on load: a preceding per-sample GroupNorm is applied on the fly, x <- x * scale[c] + shift[c] ((scale, shift) pairs of the
// insv2v_groupnorm stats_only output): the normalised copy of the activations never exists.  The sample's table is staged in LDS: the wave
// copies the 16 KS pairs (2.5 KiB at K = 320) of its 32 rows' sample once per tile - 3 loads per lane instead of 4 KS per lane from L2 - and
// every lane reads its 8 channels per k-step from there (two distinct addresses per instruction: a broadcast).  `tab` = this wave's staging
// area, tab_off = byte offset of the sample's table in rG (wave-uniform), or OOB.
// The rows of this form follow a SEGMENTED schedule, so that a wave's 32 rows share one sample for every gn_rows: each sample gets
// gn_units = ceil(gn_rows / 32) wave blocks of its own, wave block q = 4 tile + wave = (sample q / gn_units, unit q % gn_units) covers the real
// rows sample * gn_rows + unit * 32 .. + 31, and the overhang of a sample's last block (rows at or beyond gn_rows) reads zeros and is never
// stored.  One wave-uniform division per block, none per lane; the descriptors are based at the block's real first row.  With
// gn_rows % 32 == 0 this is the plain tiling of the M rows.
template <int KS>
__device__ __forceinline__ void stage_gn_table(char* tab, srd_t rG, unsigned tab_off, int lane) {
    constexpr int BYTES = 16 * KS * 8;
#pragma unroll
    for (int i = 0; i < (BYTES + 1023) / 1024; ++i) {
        const int o = i * 1024 + lane * 16;
        if (o < BYTES) {
            const uint4v v = (uint4v)__builtin_amdgcn_raw_buffer_load_b128(rG, tab_off == OOB_OFFSET ? OOB_OFFSET : tab_off + o, 0, 0);
            *(uint4v*)(tab + o) = v;
        }
    }
}
template <int KS>
__device__ __forceinline__ void gn_apply_lds(half8 (&xf)[KS], const char* tab, int half) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        floatx4 ab[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) ab[j] = *(const floatx4*)(tab + half * 64 + s * 128 + j * 16);
#pragma unroll
        for (int e = 0; e < 8; ++e) xf[s][e] = (half_t)fmaf((float)xf[s][e], ab[e >> 1][(e & 1) * 2], ab[e >> 1][(e & 1) * 2 + 1]);
    }
}
// ring depth of a row Linear: the GroupNorm-on-load form at K = 640 gives one of its nine 16 KiB slots to the four waves' (scale, shift)
// tables (4 x 5 KiB behind the ring: 148 KiB of the CU's 160)
template <int KS, bool GN>
constexpr int lin_ring_slots() { return (GN && KS > 20) ? LinCfg<KS>::NS - 1 : LinCfg<KS>::NS; }
// the geometry the planner (rows_plan.h) answers with is this file's
static_assert(LIN_SLOT_FR * 1024 == ROWLIN_SLOT_BYTES, "rows_plan.h: ring slot");
static_assert(rowlin_wgs_per_cu(20) == LinCfg<20>::WGS && rowlin_wgs_per_cu(40) == LinCfg<40>::WGS, "rows_plan.h: workgroups per CU");
static_assert(rowlin_ring_slots(20, false) == lin_ring_slots<20, false>() && rowlin_ring_slots(20, true) == lin_ring_slots<20, true>() &&
              rowlin_ring_slots(40, false) == lin_ring_slots<40, false>() && rowlin_ring_slots(40, true) == lin_ring_slots<40, true>(), "rows_plan.h: ring depth");

template <int KS, bool LN, bool FRAME, bool RES, bool GN = false, int TB = 1>
__global__ __launch_bounds__(256, LinCfg<KS>::WGS) void rowlin_kernel(RowLinArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef LinCfg<KS> Cfg;
    constexpr int GS = TB == 2 ? 4 : 8;                     // fragments per read group: at TB = 2 four fragments are eight MFMAs
    typedef Ring<LIN_SLOT_FR, lin_ring_slots<KS, GN>(), GS> R;
    constexpr int GP = Cfg::GP * (8 / GS), FR = Cfg::FR, TROWS = 128 * TB;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tok = lane & 31, half = lane >> 5;
    const int ntiles = GN ? p.gn_tiles : (p.M + TROWS - 1) / TROWS;
    const int npairs = p.N >> 6;
    R ring;
    ring.init(smem, p.wstream, npairs * (GP / R::GPS), wid, lane);

    // PF (one token block per wave): the rows of a workgroup's NEXT tile are requested right behind the last MFMA group of the current
    // one, so their HBM latency runs under the last pair's epilogue instead of in front of the next tile's first MFMA (with two token
    // blocks the 320 row registers would stay allocated through the epilogue and spill; so does the GroupNorm-on-load form - 836 bytes
    // of scratch, 2x slower - which therefore keeps its loads in front of the transform).  Measured: -2 ... -3 % per launch on the
    // LayerNorm forms (q/k/v), within noise elsewhere (profiles/r05_rowlin_prefetch.txt): the row Linears are not latency-chain bound.
    constexpr bool PF = TB == 1 && !GN;
    half8 xf[TB][KS];
    auto request_tile = [&](int t) {
        const srd_t rXn = make_srd(p.x + (int64_t)t * TROWS * p.ldx);
#pragma unroll
        for (int tb = 0; tb < TB; ++tb) {
            const int ml = (wid * TB + tb) * 32 + tok;
            const unsigned xo = (t * TROWS + ml) < p.M ? (unsigned)(((int64_t)ml * p.ldx + 8 * half) * 2) : OOB_OFFSET;
            request_rows<KS>(xf[tb], rXn, xo);
        }
    };
    if (PF && (int)blockIdx.x < ntiles) request_tile(blockIdx.x);
#pragma unroll 1
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int m[TB];
        bool mok[TB];
        unsigned xoff[TB], ooff[TB], roff[TB];
        half8 bstep[TB];
        // descriptors based at the tile's first row (64-bit), lane offsets relative to it: operands beyond 2 GiB (the fused q/k/v rows
        // of 20 stacked clips: [1 474 560, 960] fp16 = 2.8 GB) need no wider offsets
        int64_t trow0 = (int64_t)tile * TROWS;
        int gn_sample = 0, gn_u0 = 0;   // GN: the wave block's sample and its first row inside the sample
        if constexpr (GN) {              // (one token block per wave) the descriptors are the WAVE BLOCK's, based at its real first row
            const int q = tile * 4 + wid;
            gn_sample = __builtin_amdgcn_readfirstlane(q / p.gn_units);
            gn_u0 = (q - gn_sample * p.gn_units) * 32;
            trow0 = (int64_t)gn_sample * p.gn_rows + gn_u0;
        }
        const srd_t rX = make_srd(p.x + trow0 * p.ldx), rO = make_srd(p.out + trow0 * p.ldo),
                    rR = make_srd(RES ? (const void*)(p.residual + trow0 * p.ldr) : (const void*)p.x);
#pragma unroll
        for (int tb = 0; tb < TB; ++tb) {
            const int ml = GN ? tok : (wid * TB + tb) * 32 + tok;
            if constexpr (GN) {   // (a spare block of the last tile starts at or beyond M)
                m[tb] = (int)trow0 + ml;
                mok[tb] = gn_u0 + tok < p.gn_rows && trow0 + ml < p.M;
            } else {
                m[tb] = tile * TROWS + ml;
                mok[tb] = m[tb] < p.M;
            }
            xoff[tb] = mok[tb] ? (unsigned)(((int64_t)ml * p.ldx + 8 * half) * 2) : OOB_OFFSET;
            ooff[tb] = mok[tb] ? (unsigned)(((int64_t)ml * p.ldo + 8 * half) * 2) : OOB_OFFSET;
            roff[tb] = (RES && mok[tb]) ? (unsigned)(((int64_t)ml * p.ldr + 8 * half) * 2) : OOB_OFFSET;
            if constexpr (GN) {
                // a wave's 32 rows share one sample (the segmented schedule): its table goes through this wave's 16 KS * 8 bytes behind the ring
                char* tab = smem + R::NS * R::SLOT_B + (wid * TB + tb) * (16 * KS * 8);
                const unsigned toff = trow0 < p.M ? (unsigned)((int64_t)gn_sample * (16 * KS) * 8) : OOB_OFFSET;
                stage_gn_table<KS>(tab, make_srd(p.gn_ab), toff, lane);
                request_rows<KS>(xf[tb], rX, xoff[tb]);
                gn_apply_lds<KS>(xf[tb], tab, half);
            } else if (!PF) {
                request_rows<KS>(xf[tb], rX, xoff[tb]);
            }
            if (LN) layernorm_frags<KS>(xf[tb], p.eps);
            // (The row fragments are B operands of every MFMA of the tile, and the allocator moves part of them to accumulator registers and
            // back, four v_accvgpr_read per use.  Pinning them there was measured slower - the LayerNorm form lost 38 % - and is gone:
            // profiles/r05_rows_pin_agpr.txt.)
            // B fragment of the bias k-step: ones, or the one-hot of the token's frame against the per-frame table
            if (FRAME) bstep[tb] = frame_hot(mok[tb] ? (m[tb] / p.rows_per_frame) % p.frames : 0, half);
            else bstep[tb] = bias_ones(half);
        }

        floatx16 acc0[TB], acc1[TB];
        uint4v resv[TB][2][2];
        half8 fb[2][GS];
        // group g of a pair section: fragments GS g .. GS g + GS - 1; fragment f = (k-step f >> 1, tile f & 1) for f < FR.  TB = 2: every
        // weight fragment read from LDS feeds TWO MFMAs (the wave's two 32-token blocks)
        auto consume_group = [&](auto g_) {
            constexpr int g = decltype(g_)::value;
#pragma unroll
            for (int i = 0; i < GS; ++i) {
                const int f = g * GS + i;
                if (f < FR) {
                    const int s = f >> 1;
#pragma unroll
                    for (int tb = 0; tb < TB; ++tb) {
                        const half8 b = s < KS ? xf[tb][s < KS ? s : 0] : bstep[tb];
                        if (f == 0) zero16(acc0[tb]);
                        if (f == 1) zero16(acc1[tb]);
                        if (f & 1) acc1[tb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[g & 1][i], b, acc1[tb], 0, 0, 0);
                        else acc0[tb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fb[g & 1][i], b, acc0[tb], 0, 0, 0);
                    }
                }
                if (i == 3) ring.template refill<g % R::GPS, 0>();
                if (GS == 8 && i == 7) ring.template refill<g % R::GPS, 1>();
            }
        };
        auto prefetch_res = [&](int pair) {
#pragma unroll
            for (int tb = 0; tb < TB; ++tb) {
                load_res_tile<RES>(resv[tb][0], rR, roff[tb], pair * 128);
                load_res_tile<RES>(resv[tb][1], rR, roff[tb], pair * 128 + 64);
            }
        };
        float st1[TB], st2[TB];
#pragma unroll
        for (int tb = 0; tb < TB; ++tb) { st1[tb] = 0.f; st2[tb] = 0.f; }
        const bool want_stats = p.stats != nullptr;   // wave-uniform
        auto epilogue = [&](int pair) {   // tiles 2 pair, 2 pair + 1
#pragma unroll
            for (int tb = 0; tb < TB; ++tb) {
                store_tile<RES>(acc0[tb], resv[tb][0], rO, ooff[tb], pair * 128, want_stats ? &st1[tb] : nullptr, want_stats ? &st2[tb] : nullptr);
                store_tile<RES>(acc1[tb], resv[tb][1], rO, ooff[tb], pair * 128 + 64, want_stats ? &st1[tb] : nullptr, want_stats ? &st2[tb] : nullptr);
            }
        };
#pragma unroll 1
        for (int pr = 0; pr < npairs; ++pr) {
            ring.template read_group<0>(fb[0]);
            if (pr > 0) { consume_group(ic<GP - 1>{}); epilogue(pr - 1); }   // (the pass's first pair has no predecessor; its refill phase
                                                                            //  is the one of the final consume_group below)
            prefetch_res(pr);
            static_for<GP - 1>([&](auto g_) {
                constexpr int g = decltype(g_)::value;
                ring.template read_group<g + 1>(fb[(g + 1) & 1]);
                consume_group(ic<g>{});
            });
        }
        consume_group(ic<GP - 1>{});
        if (PF && tile + (int)gridDim.x < ntiles) request_tile(tile + gridDim.x);
        epilogue(npairs - 1);
        if (want_stats) {   // every output element of a token was stored by exactly one of its two lanes
#pragma unroll
            for (int tb = 0; tb < TB; ++tb) {
                const float s1 = st1[tb] + __shfl_xor(st1[tb], 32, 64), s2 = st2[tb] + __shfl_xor(st2[tb], 32, 64);
                const float mean = s1 / p.N;
                if (half == 0 && mok[tb]) ((float2*)p.stats)[m[tb]] = make_float2(mean, rsqrtf(fmaxf(s2 / p.N - mean * mean, 0.f) + p.stats_eps));
            }
        }
    }
    wait_vmcnt<0>();
}

}  // namespace

extern "C" int insv2v_ffn_fused(const insv2v_ffn_desc* dp, insv2v_stream_t stream) {
    if (!one_device()) return INSV2V_EINVAL;
    if (!dp) return INSV2V_EINVAL;
    const insv2v_ffn_desc& d = *dp;
    if (!d.x || !d.out || !d.wstream || d.M <= 0) return INSV2V_EINVAL;
    if (d.C != FC || d.hidden != 4 * FC) return INSV2V_EUNSUPPORTED;
    if ((d.ldx & 7) || (d.ldo & 7) || ((uintptr_t)d.x & 15) || ((uintptr_t)d.out & 15) || ((uintptr_t)d.wstream & 15)) return INSV2V_EINVAL;
    if (d.post && (!d.post_residual || (d.ld_post & 7) || ((uintptr_t)d.post_residual & 15))) return INSV2V_EINVAL;
    const FfnArgs a = {(const half_t*)d.x, (half_t*)d.out, (const half_t*)d.wstream, (const half_t*)d.post_residual, d.ldx, d.ldo, d.ld_post, d.M, d.eps};
    // x, out and post_residual may each exceed the 2 GiB window: ranges of whole 128-row tiles, one launch each (launch_unit_ranges)
    const int64_t ld = std::max(std::max(d.ldx, d.ldo), d.post ? d.ld_post : (int64_t)0);
    return launch_unit_ranges(((int64_t)d.M + 127) / 128, 128 * ld * 2, [&](int64_t t0, int64_t nt) {
        FfnArgs r = a;
        const int64_t m0 = t0 * 128;
        r.x += m0 * a.ldx; r.out += m0 * a.ldo;
        if (d.post) r.res2 += m0 * a.ldr2;
        r.M = (int)std::min(nt * 128, (int64_t)d.M - m0);
        static bool post_attr = false, attr_set = false;
        if (d.post) return launch_rows((const void*)ffn_fused_kernel<true>, post_attr, FFN_NS * FFN_SLOT_FR * 1024, r, r.M, as_stream(stream));
        return launch_rows((const void*)ffn_fused_kernel<false>, attr_set, FFN_NS * FFN_SLOT_FR * 1024, r, r.M, as_stream(stream));
    }, (int64_t)d.M * ld * 2);
}

// Size in fp16 elements of the weight stream insv2v_ffn_fused expects for (C, hidden); 0 if unsupported.
extern "C" int64_t insv2v_ffn_stream_elems(int32_t C, int32_t hidden, int32_t post) {
    if (C != FC || hidden != 4 * FC) return 0;
    return (int64_t)(FFN_PASS_SLOTS + (post ? FFN_POST_SLOTS : 0)) * FFN_SLOT_FR * 512;
}

// The kernel the plan names (rows_plan.h): form = LN << 2 | FRAME << 1 | RES, the GroupNorm-on-load form, one or two token blocks per wave
template <int KS>
static int launch_rowlin(const insv2v_rowlin_plan_t& pl, const RowLinArgs& a, hipStream_t s) {
    static const void* kernels[8] = {(const void*)rowlin_kernel<KS, false, false, false>, (const void*)rowlin_kernel<KS, false, false, true>,
                                     (const void*)rowlin_kernel<KS, false, true, false>, (const void*)rowlin_kernel<KS, false, true, true>,
                                     (const void*)rowlin_kernel<KS, true, false, false>, (const void*)rowlin_kernel<KS, true, false, true>,
                                     (const void*)rowlin_kernel<KS, true, true, false>, (const void*)rowlin_kernel<KS, true, true, true>};
    static bool attr_set[8] = {};
    const int v = pl.form;
    if (pl.gn) {   // fused input GroupNorm: only the plain form (proj_in of the transformer blocks) exists
        static bool gn_attr = false;
        return launch_grid((const void*)rowlin_kernel<KS, false, false, false, true>, gn_attr, pl.lds_bytes, a, pl.grid, s);
    }
    if constexpr (KS == 40) {   // two token blocks per wave where the register file holds them
        static const void* k2[8] = {(const void*)rowlin_kernel<KS, false, false, false, false, 2>, (const void*)rowlin_kernel<KS, false, false, true, false, 2>,
                                    (const void*)rowlin_kernel<KS, false, true, false, false, 2>, (const void*)rowlin_kernel<KS, false, true, true, false, 2>,
                                    (const void*)rowlin_kernel<KS, true, false, false, false, 2>, (const void*)rowlin_kernel<KS, true, false, true, false, 2>,
                                    (const void*)rowlin_kernel<KS, true, true, false, false, 2>, (const void*)rowlin_kernel<KS, true, true, true, false, 2>};
        static bool attr2[8] = {};
        if (pl.token_blocks == 2) return launch_grid(k2[v], attr2[v], pl.lds_bytes, a, pl.grid, s);
    }
    if (pl.token_blocks != 1) return INSV2V_EINVAL;
    return launch_grid(kernels[v], attr_set[v], pl.lds_bytes, a, pl.grid, s);
}

// bit v of the mask: form v runs two token blocks per wave at K = 640 (INSV2V_ROWLIN_TB2 overrides, for A/B); read once for the library
static int rowlin_tb2_mask() {
    static const int tb2 = getenv("INSV2V_ROWLIN_TB2") ? atoi(getenv("INSV2V_ROWLIN_TB2")) : ROWLIN_TB2_DEFAULT;
    return tb2;
}

// ONE planner (rows_plan.h) answers for the launch and for the read-only entry, so that they cannot disagree
extern "C" int insv2v_rowlin_plan(const insv2v_rowlin_desc* dp, int32_t cus, insv2v_rowlin_plan_t* out) {
    if (!dp || !out) return INSV2V_EINVAL;
    *out = plan_rowlin(*dp, rowlin_tb2_mask(), cus > 0 ? cus : insv2v_num_cus());
    return 0;
}

extern "C" int insv2v_rowlin(const insv2v_rowlin_desc* dp, insv2v_stream_t stream) {
    if (!one_device()) return INSV2V_EINVAL;
    if (!dp) return INSV2V_EINVAL;
    const insv2v_rowlin_desc& d = *dp;
    const insv2v_rowlin_plan_t pl = plan_rowlin(d, rowlin_tb2_mask(), num_cus());
    if (pl.rc) return pl.rc;
    const RowLinArgs a = {(const half_t*)d.x, (half_t*)d.out, (const half_t*)d.residual, (const half_t*)d.wstream, d.ldx, d.ldo, d.ldr,
                          d.M, d.N, d.rows_per_frame, d.frames, d.eps, d.stats_out, d.stats_eps, d.gn_ab, d.gn_rows, pl.gn_units, pl.gn ? pl.ntiles : 0};
    return pl.ks == 20 ? launch_rowlin<20>(pl, a, as_stream(stream)) : launch_rowlin<40>(pl, a, as_stream(stream));
}

// fp16 elements of the weight stream insv2v_rowlin expects for a [N, K] Linear; 0 if unsupported
extern "C" int64_t insv2v_rowlin_stream_elems(int32_t N, int32_t K) {
    if (!rowlin_k_ok(K) || N <= 0 || (N & 63)) return 0;
    const int gp = K == 320 ? LinCfg<20>::GP : LinCfg<40>::GP;
    return (int64_t)(N >> 6) * gp * 8 * 512;
}
