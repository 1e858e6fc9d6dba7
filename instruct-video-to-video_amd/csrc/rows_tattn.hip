// Fused temporal attention: insv2v_tattn_fused (C = 320) and insv2v_tattn_attn (C = 640); the register-resident scheme: rows_common.h
#include "rows_common.h"
#include <algorithm>

namespace {
// ===================================================================================================== temporal attention block
// insv2v_tattn_fused: one TemporalTransformerBlock attention sub-block (motion_module.py:270-336 behind the LayerNorm of :206) at
// C = 320, 8 heads x 40, a window of 1 .. 32 frames, as ONE register-resident launch:
//     out = x + Wo . Attn_over_frames( LayerNorm(x) Wqkv^T + (beta, positional-encoding) bias ) + bo
// A wave owns 2 pixels x 16 frame slots = 32 tokens (FP = 16: windows of 1 .. 16 frames) or 1 pixel x 32 frame slots (FP = 32: 17 .. 32
// frames) - rows (b, f, p) of the token matrix: the frame axis is a row stride of HW.  q, k and v tiles come out of the MFMAs in the C
// layout, and every later contraction reads them as an operand IN PLACE:
//   * q^T / k^T tiles ([32 channels] x [32 tokens]) packed to fp16 are legal B / A fragments of S^T = K . Q^T for a permuted channel
//     order (any order works, it is a contraction index); a head is 40 channels = 5 "octets" (8 channels = one register quad of both
//     lane halves): two full k-steps + one half-zero k-step (only the Q side is masked);
//   * FP = 16: S^T is 32 keys x 32 queries: the 16 x 16 diagonal blocks are the two pixels, the rest is discarded by a register select on
//     the query's pixel; softmax over 16 keys = 8 in-lane values + one exchange with the other lane half.  FP = 32: S^T is the pixel's
//     whole 32 x 32 block; softmax over 32 keys = all 16 in-lane values (key rows (r & 3) + 8 (r >> 2) + 4 half) + one exchange;
//   * V is computed with the MFMA operands swapped ([tokens] x [channels]), which makes its packed tile the A fragment of
//     O^T = V^T . P^T (k = keys, in exactly the order the probabilities sit in the lane); FP = 16: P of the other pixel's keys is zero,
//     FP = 32: PB[h][0] / [1] are the probabilities of key rows 0-15 / 16-31, the two k-steps of the packed V tile;
//   * O^T tiles ([channels] x [queries]) normalised by 1 / l and packed are the B fragments of the output projection.
// A window shorter than its FP slots (MASKED): frame slots >= F are neither loaded (zero rows: LayerNorm gives zeros) nor stored, and
// their residual is not read; their KEYS would still score (a zero row's key is its table row, zero: score 0, not -inf), so keys >= F
// get -1e30 before the maximum and probability exactly 0 - the row sum l covers the valid keys only.
// Weight stream (insv2v/fused.py pack_tattn_stream), NB = FP / 16 one-hot frame-bias k-steps per q/k/v tile (KSB = 20 + NB k-steps):
//   for head group G = 0, 1 (4 heads = 5 channel tiles): [Q/K of tile tl, k-step s: (q, k)] x 5 x KSB | [V pair (0,1)] [V pair (2,3)] [V 4]
//   | pad to a whole slot (NB = 1: 315 + 5 = 320 fragments, NB = 2: 330 + 6 = 336);  [output tiles in pairs x 21] | pad 14;
//   k-steps 20 .. 20 + NB - 1 = the bias steps (per-frame table rows 16 j .. 16 j + 15 for q/k/v, plain bias for the output).
//   NB = 1: 864 fragments = 54 slots per pass, NB = 2: 896 = 56 slots.
struct TattnArgs {
    const half_t* x;
    half_t* out;
    const half_t* wstream;
    int64_t ldx, ldo;
    int HW, npix;          // pixels per sample, total pixels (samples x HW); rows = npix x frames
    float eps, scale;
};
constexpr int TA_H = 8, TA_F = 16;   // heads (40 channels each at C = 320, 80 at C = 640); frames of the unmasked kernels
struct TattnWinArgs : TattnArgs {   // the masked forms: + the window length F (1 .. FP)
    int frames;
};
template <bool MASKED> using TattnArgsT = std::conditional_t<MASKED, TattnWinArgs, TattnArgs>;
__device__ __forceinline__ int win_frames(const TattnArgs&) { return TA_F; }
__device__ __forceinline__ int win_frames(const TattnWinArgs& p) { return p.frames; }
constexpr int TA_SEC_O = 224;                          // fragment positions of the output-projection section
// section sizes for NB frame-bias steps per q/k/v tile
template <int NB> struct TaSched {
    static constexpr int KSB = KS1 + NB, QK = 10 * KSB, VP = 4 * KSB, SEC_G = (QK + VP + KSB + 15) / 16 * 16, TOTAL = 2 * SEC_G + TA_SEC_O;
};
static_assert(TaSched<1>::SEC_G == 320 && TaSched<1>::TOTAL == 864, "the 16-frame stream is unchanged");
struct TaOp { int kind, G, t, s; };   // kind 0 pad, 1 Q, 2 K, 3 V (t = local tile 0..4), 4 OUT (t = output tile 0..9)
template <int NB>
constexpr TaOp ta_op(int f) {
    typedef TaSched<NB> S;
    if (f < 2 * S::SEC_G) {
        const int G = f / S::SEC_G;
        int r = f % S::SEC_G;
        if (r < S::QK) return {1 + (r % (2 * S::KSB) & 1), G, r / (2 * S::KSB), (r % (2 * S::KSB)) >> 1};
        r -= S::QK;
        if (r < S::VP) return {3, G, 2 * (r / (2 * S::KSB)) + (r % (2 * S::KSB) & 1), (r % (2 * S::KSB)) >> 1};
        r -= S::VP;
        if (r < S::KSB) return {3, G, 4, r};
        return {0, 0, 0, 0};
    }
    const int r = f - 2 * S::SEC_G;
    if (r < 210) return {4, 0, 2 * (r / 42) + (r % 42 & 1), (r % 42) >> 1};
    return {0, 0, 0, 0};
}

// Frame-bias operands: fhot = the one-hot of the token's frame over frames 0 .. 15 (lane half h holds frames 8 h .. 8 h + 7); with NB = 2
// frame-bias steps, frame_hot1 is the one-hot over frames 16 .. 31 (lane half h: 16 + 8 h .. + 7), zero otherwise (unused).
// (fhot itself is spelled out in both kernels, not frame_hot(fr, half): through the call hipcc orders the two compares the other way
// round and from there allocates the registers of the whole kernel differently - tattn_fused_kernel<16, true> 502 -> 510.)
template <int NB>
__device__ __forceinline__ half8 frame_hot1(int fr, int half) {
    if constexpr (NB > 1) return frame_hot(fr, 2 + half);
    return half8{0, 0, 0, 0, 0, 0, 0, 0};
}
// Scheduler pipeline behind every fragment group of the two kernels: one MFMA, then up to TA_SGB of whatever VALU work sits in the group's
// region, eight times.  N = 3 gains 2.5 / 3.8 % per launch (profiles/r05_rows_sched_pipelines.txt; the text cross-attention kernels gain
// nothing with N = 3 and lose 1 % with N = 5, so they have none).
constexpr int TA_SGB = 3;
__device__ __forceinline__ void tattn_group_pipeline() {
#pragma unroll
    for (int i = 0; i < 8; ++i) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(0x002, TA_SGB, 0); }
}

// Softmax of one head's S^T tile for the lane's query -> probabilities packed as the two key k-steps of O^T = V^T . P^T, and 1 / l.
// FP = 16: the block of the query's pixel pp (8 in-lane values, block-local key rows (j & 3) + 8 (j >> 2) + 4 half); the other pixel's
// k-step is zero.  FP = 32: all 16 in-lane values (key rows (j & 3) + 8 (j >> 2) + 4 half).  MASKED: keys >= F, i.e. in-lane key row
// (j & 3) + 8 (j >> 2) >= klim = F - 4 half, get -1e30: they do not set the maximum and their exp2 is exactly 0.
// (The two unmasked 16-frame kernels carried their own copy of the <16, false> case until this function replaced it; that changed their
// schedule by a few instructions and was accepted on a measurement: profiles/rows_refactor_tattn16_ab.txt.)
template <int FP, bool MASKED>
__device__ __forceinline__ void tattn_softmax(const floatx16& S, int pp, int klim, float c2, half8 (&PB)[2], float& invl) {
    constexpr int N = FP / 2;
    float sel[N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if constexpr (FP == 16) { const float s0 = S[j], s1 = S[8 + j]; sel[j] = pp ? s1 : s0; }
        else sel[j] = S[j];
        if constexpr (MASKED) sel[j] = (j & 3) + 8 * (j >> 2) < klim ? sel[j] : -1e30f;
    }
    float mx = sel[0];
#pragma unroll
    for (int j = 1; j < N; ++j) mx = fmaxf(mx, sel[j]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mc = -mx * c2;
    float e[N];
#pragma unroll
    for (int j = 0; j < N; ++j) e[j] = __builtin_amdgcn_exp2f(fmaf(sel[j], c2, mc));
    half8 pe[N / 8];
#pragma unroll
    for (int k = 0; k < N / 8; ++k) {
        const uint4v u = {pk2(e[8 * k], e[8 * k + 1]), pk2(e[8 * k + 2], e[8 * k + 3]), pk2(e[8 * k + 4], e[8 * k + 5]), pk2(e[8 * k + 6], e[8 * k + 7])};
        pe[k] = __builtin_bit_cast(half8, u);
    }
    float l = 0.f;
#pragma unroll
    for (int k = 0; k < N / 8; ++k)
#pragma unroll
        for (int j = 0; j < 8; ++j) l += (float)pe[k][j];             // the ROUNDED probabilities, as the P.V MFMAs see them
    l += __shfl_xor(l, 32, 64);
    invl = 1.f / l;
    if constexpr (FP == 16) {
        const half8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        PB[0] = pp ? zero8 : pe[0];
        PB[1] = pp ? pe[0] : zero8;
    } else {
        PB[0] = pe[0];
        PB[1] = pe[1];
    }
}

template <int FP, bool MASKED>
__global__ __launch_bounds__(256, 1) void tattn_fused_kernel(TattnArgsT<MASKED> p) {
    static_assert(FP == 16 || (FP == 32 && MASKED), "FP = 32 always masks (windows of 17 .. 32 frames)");
    constexpr int NB = FP / 16, PPW = 32 / FP;        // frame-bias k-steps, pixels per wave
    typedef TaSched<NB> SC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef Ring<16, 9> R;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tok = lane & 31, half = lane >> 5;
    const int pp = FP == 16 ? tok >> 4 : 0, fr = FP == 16 ? tok & 15 : tok;   // pixel of the wave's pair, frame
    const int F = win_frames(p);
    const int ntiles = (p.npix + 4 * PPW - 1) / (4 * PPW);
    const srd_t rX = make_srd(p.x), rO = make_srd(p.out);
    R ring;
    ring.init(smem, p.wstream, SC::TOTAL / 16, wid, lane);

    const half8 ones = bias_ones(half);
    half8 fhot = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; ++e) fhot[e] = (half == (fr >> 3) && e == (fr & 7)) ? (half_t)1.f : (half_t)0.f;
    const half8 fhot1 = frame_hot1<NB>(fr, half);
    const int klim = F - 4 * half;
    const float c2 = p.scale * 1.4426950408889634f;

#pragma unroll 1
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int pix = tile * 4 * PPW + wid * PPW + pp;
        const bool mok = pix < p.npix && (!MASKED || fr < F);
        const int b = pix / p.HW, pl = pix - b * p.HW;
        const int64_t m = ((int64_t)b * F + fr) * p.HW + pl;
        const unsigned xoff = mok ? (unsigned)((m * p.ldx + 8 * half) * 2) : OOB_OFFSET;
        const unsigned ooff = mok ? (unsigned)((m * p.ldo + 8 * half) * 2) : OOB_OFFSET;
        half8 xn[KS1];
        load_rows<KS1, true>(xn, rX, xoff, p.eps);

        half8 afr[KS1];                    // attention output, packed: the B fragments of the output projection
        half8 qs[10], ks[10];              // q / k of the current head group, packed per k-step (2 octets each)
        half8 PB[4][2];                    // probabilities of the group's 4 heads: [key k-step 0 | 1]
        float invl[4];
        floatx16 acc0, acc1;               // Q / K, V pair, output pair
        uint4v resv[2][2];
        half8 fb[2][8];

        // ---- per-group attention scores -> PB, invl
        auto scores = [&]() {
            floatx16 S[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) zero16(S[h]);
            // step 0 / 1: the two full k-steps, step 2: the single octet (Q side half-zero); heads interleaved: 4 independent MFMA chains
            static_for<3>([&](auto st_) {
                static_for<4>([&](auto h_) {
                    constexpr int st = decltype(st_)::value, h = decltype(h_)::value;
                    constexpr int lo = 5 * h;                               // first octet of the head within the group
                    if constexpr (st < 2) {
                        constexpr int kst = (lo & 1) ? (lo + 1) / 2 + st : lo / 2 + st;
                        S[h] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ks[kst], qs[kst], S[h], 0, 0, 0);
                    } else {
                        constexpr int o = (lo & 1) ? lo : lo + 4;           // the unpaired octet
                        constexpr int kst = o >> 1;
                        uint4v u = __builtin_bit_cast(uint4v, qs[kst]);
                        if (o & 1) { u[0] = 0; u[1] = 0; } else { u[2] = 0; u[3] = 0; }
                        S[h] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ks[kst], __builtin_bit_cast(half8, u), S[h], 0, 0, 0);
                    }
                });
            });
#pragma unroll
            for (int h = 0; h < 4; ++h) tattn_softmax<FP, MASKED>(S[h], pp, klim, c2, PB[h], invl[h]);
        };
        // ---- O^T of local tile tl of group G from its packed V tile -> afr
        auto pv_tile = [&](auto G_, auto tl_, const floatx16& accV) {
            constexpr int G = decltype(G_)::value, tl = decltype(tl_)::value;
            constexpr int ha = (4 * tl) / 5, hb = (4 * tl + 3) / 5;
            half8 v0, v1;
            pack_tile(accV, v0, v1);
            floatx16 Oa, Ob;
            zero16(Oa);
            Oa = __builtin_amdgcn_mfma_f32_32x32x16_f16(v0, PB[ha][0], Oa, 0, 0, 0);
            Oa = __builtin_amdgcn_mfma_f32_32x32x16_f16(v1, PB[ha][1], Oa, 0, 0, 0);
            if (hb != ha) {
                zero16(Ob);
                Ob = __builtin_amdgcn_mfma_f32_32x32x16_f16(v0, PB[hb][0], Ob, 0, 0, 0);
                Ob = __builtin_amdgcn_mfma_f32_32x32x16_f16(v1, PB[hb][1], Ob, 0, 0, 0);
            }
            floatx16 o;
#pragma unroll
            for (int qd = 0; qd < 4; ++qd) {
                const int h = (4 * tl + qd) / 5;
#pragma unroll
                for (int e = 0; e < 4; ++e) o[4 * qd + e] = (h == ha ? Oa[4 * qd + e] : Ob[4 * qd + e]) * invl[h];
            }
            pack_tile(o, afr[2 * (5 * G + tl)], afr[2 * (5 * G + tl) + 1]);
        };

        auto consume_group = [&](auto g_) {
            constexpr int g = decltype(g_)::value;
            static_for<8>([&](auto i_) {
                constexpr int i = decltype(i_)::value, f = g * 8 + i;
                constexpr TaOp op = ta_op<NB>(f);
                const half8 a = fb[g & 1][i];
                if constexpr (op.kind == 1 || op.kind == 2) {          // q / k tile of the group: A = weights, B = tokens
                    const half8 bop = op.s < KS1 ? xn[op.s < KS1 ? op.s : 0] : op.s == KS1 ? fhot : fhot1;
                    if constexpr (op.kind == 1) {
                        if (op.s == 0) zero16(acc0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc0, 0, 0, 0);
                    } else {
                        if (op.s == 0) zero16(acc1);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc1, 0, 0, 0);
                        if constexpr (op.s == SC::KSB - 1) {            // tile complete
                            pack_tile(acc0, qs[2 * op.t], qs[2 * op.t + 1]);
                            pack_tile(acc1, ks[2 * op.t], ks[2 * op.t + 1]);
                            if constexpr (op.t == 4) scores();
                        }
                    }
                } else if constexpr (op.kind == 3) {                    // v tile, operands swapped: A = tokens, B = weights -> [token][channel]
                    const half8 aop = op.s < KS1 ? xn[op.s < KS1 ? op.s : 0] : op.s == KS1 ? fhot : fhot1;
                    constexpr bool second = op.t == 1 || op.t == 3;
                    if constexpr (second) {
                        if (op.s == 0) zero16(acc1);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(aop, a, acc1, 0, 0, 0);
                        if constexpr (op.s == SC::KSB - 1) { pv_tile(ic<op.G>{}, ic<op.t - 1>{}, acc0); pv_tile(ic<op.G>{}, ic<op.t>{}, acc1); }
                    } else {
                        if (op.s == 0) zero16(acc0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(aop, a, acc0, 0, 0, 0);
                        if constexpr (op.s == SC::KSB - 1 && op.t == 4) pv_tile(ic<op.G>{}, ic<4>{}, acc0);
                    }
                } else if constexpr (op.kind == 4) {                    // output projection, tiles in pairs
                    const half8 bop = op.s < KS1 ? afr[op.s < KS1 ? op.s : 0] : ones;
                    if constexpr ((op.t & 1) == 0) {
                        if (op.s == 0) { zero16(acc0); load_res_tile<true>(resv[0], rX, xoff, op.t * 64); load_res_tile<true>(resv[1], rX, xoff, op.t * 64 + 64); }
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc0, 0, 0, 0);
                    } else {
                        if (op.s == 0) zero16(acc1);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc1, 0, 0, 0);
                        if constexpr (op.s == KS1) {
                            store_tile<true>(acc0, resv[0], rO, ooff, (op.t - 1) * 64);
                            store_tile<true>(acc1, resv[1], rO, ooff, op.t * 64);
                        }
                    }
                }
                if (i == 3) ring.template refill<g % R::GPS, 0>();
                if (i == 7) ring.template refill<g % R::GPS, 1>();
            });
            tattn_group_pipeline();
        };
        constexpr int NG = SC::TOTAL / 8;   // 108 (FP = 16) / 112 (FP = 32) groups per pass
        ring.template read_group<0>(fb[0]);
        static_for<NG - 1>([&](auto g_) {
            constexpr int g = decltype(g_)::value;
            ring.template read_group<g + 1>(fb[(g + 1) & 1]);
            consume_group(ic<g>{});
        });
        consume_group(ic<NG - 1>{});
    }
    wait_vmcnt<0>();
}

}  // namespace

// Both launchers: validation, the argument block, and the pick of one of three kernels - 16 frames: the unmasked kernel; 1 .. 15: 16
// frame slots with the tail masked; 17 .. 32: 32 frame slots, one pixel per wave
static int launch_tattn(const insv2v_tattn_desc* dp, int C, const void* const (&kernels)[3], bool (&attr_set)[3], insv2v_stream_t stream) {
    if (!one_device()) return INSV2V_EINVAL;
    if (!dp) return INSV2V_EINVAL;
    const insv2v_tattn_desc& d = *dp;
    if (!d.x || !d.out || !d.wstream || d.samples <= 0 || d.HW <= 0) return INSV2V_EINVAL;
    if (d.C != C || d.heads != TA_H || d.frames < 1 || d.frames > 32) return INSV2V_EUNSUPPORTED;
    if ((d.ldx & 7) || (d.ldo & 7) || ((uintptr_t)d.x & 15) || ((uintptr_t)d.out & 15) || ((uintptr_t)d.wstream & 15)) return INSV2V_EINVAL;
    const int v = d.frames == TA_F ? 0 : d.frames < TA_F ? 1 : 2, FP = v == 2 ? 32 : 16;
    // x and out may each exceed the 2 GiB window: ranges of whole samples, one launch each (launch_unit_ranges; a wave never reads across
    // a sample, so one sample's frames x HW rows are what has to fit)
    const int64_t srows = (int64_t)d.frames * d.HW;
    return launch_unit_ranges(d.samples, srows * std::max(d.ldx, d.ldo) * 2, [&](int64_t s0, int64_t ns) {
        if (ns * d.HW * FP > 0x7fffffff) return (int)INSV2V_EUNSUPPORTED;
        TattnWinArgs a;
        static_cast<TattnArgs&>(a) = {(const half_t*)d.x + s0 * srows * d.ldx, (half_t*)d.out + s0 * srows * d.ldo, (const half_t*)d.wstream,
                                      d.ldx, d.ldo, d.HW, (int)(ns * d.HW), d.eps, d.scale};
        a.frames = d.frames;
        // launch_rows sizes the grid from a row count in 128-row tiles: a tile here is 8 pixels x 16 frame slots or 4 pixels x 32 = 128 rows
        const int M = a.npix * FP;
        if (v == 0) return launch_rows(kernels[0], attr_set[0], 9 * 16 * 1024, static_cast<const TattnArgs&>(a), M, as_stream(stream));
        return launch_rows(kernels[v], attr_set[v], 9 * 16 * 1024, a, M, as_stream(stream));
    });
}

extern "C" int insv2v_tattn_fused(const insv2v_tattn_desc* dp, insv2v_stream_t stream) {
    static const void* const kernels[3] = {(const void*)tattn_fused_kernel<16, false>, (const void*)tattn_fused_kernel<16, true>, (const void*)tattn_fused_kernel<32, true>};
    static bool attr_set[3] = {};
    return launch_tattn(dp, FC, kernels, attr_set, stream);
}

// fp16 elements of the stream for a window of `frames` (1 .. 16: 16 frame slots, 17 .. 32: 32); 0 if unsupported
extern "C" int64_t insv2v_tattn_stream_elems(int32_t C, int32_t heads, int32_t frames) {
    if (C != FC || heads != TA_H || frames < 1 || frames > 32) return 0;
    return (int64_t)(frames <= TA_F ? TaSched<1>::TOTAL : TaSched<2>::TOTAL) * 512;
}

namespace {
// ===================================================================================================== temporal attention, C = 640
// insv2v_tattn_attn: LayerNorm -> (+pe) -> q/k/v -> attention over the 1 .. 32 frames of every pixel at C = 640 (8 heads x 80), WITHOUT the
// output projection: 640 channels of activations (160 registers) + the packed attention output for a K = 640 projection (160 more) do not fit
// next to the working set, so the attention output [rows, 640] goes to memory and insv2v_rowlin adds to_out + residual.  q, k and v (a
// [rows, 1920] tensor written and re-read per block before) never exist in memory.  Same scheme, frame slots (FP = 16 / 32) and window
// masking as tattn_fused_kernel; a head is 80 channels = 5 whole k-steps of a 160-channel group (2 heads per group, 4 groups), so no channel
// is masked.  One group's weights = 624 (FP = 16) / 640 (FP = 32) fragments = 39 / 40 ring slots; the group loop is a run-time loop around
// one unrolled group body (the instruction stream of four would not stay in the instruction cache).
// Stream per group G (channel tiles c = 5G .. 5G+4), NB = FP / 16 frame-bias steps (k-steps 40 .. 40 + NB - 1):
//   [tile c: k-step s = 0 .. 39 + NB: (q, k)] x 5 | [v pair (5G, 5G+1)] [v pair (5G+2, 5G+3)] [v 5G+4] | pad 9 (NB = 1) / 10 (NB = 2)
constexpr int TB_KS = 40;
template <int NB> struct TbSched {
    static constexpr int KSB = TB_KS + NB, QK = 10 * KSB, VP = 4 * KSB, GROUP_FR = (QK + VP + KSB + 15) / 16 * 16;
};
static_assert(TbSched<1>::GROUP_FR == 624, "the 16-frame stream is unchanged");
struct TbOp { int kind, t, s; };   // kind 0 pad, 1 Q, 2 K, 3 V (t = local tile 0..4)
template <int NB>
constexpr TbOp tb_op(int r) {
    typedef TbSched<NB> S;
    if (r < S::QK) return {1 + (r % (2 * S::KSB) & 1), r / (2 * S::KSB), (r % (2 * S::KSB)) >> 1};
    r -= S::QK;
    if (r < S::VP) return {3, 2 * (r / (2 * S::KSB)) + (r % (2 * S::KSB) & 1), (r % (2 * S::KSB)) >> 1};
    r -= S::VP;
    if (r < S::KSB) return {3, 4, r};
    return {0, 0, 0};
}

template <int FP, bool MASKED>
__global__ __launch_bounds__(256, 1) void tattn640_kernel(TattnArgsT<MASKED> p) {
    static_assert(FP == 16 || (FP == 32 && MASKED), "FP = 32 always masks (windows of 17 .. 32 frames)");
    constexpr int NB = FP / 16, PPW = 32 / FP;
    typedef TbSched<NB> SC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    typedef Ring<16, 9> R;
    constexpr int KS = TB_KS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tok = lane & 31, half = lane >> 5;
    const int pp = FP == 16 ? tok >> 4 : 0, fr = FP == 16 ? tok & 15 : tok;
    const int F = win_frames(p);
    const int ntiles = (p.npix + 4 * PPW - 1) / (4 * PPW);
    const srd_t rX = make_srd(p.x), rO = make_srd(p.out);
    R ring;
    ring.init(smem, p.wstream, 4 * SC::GROUP_FR / 16, wid, lane);

    half8 fhot = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 8; ++e) fhot[e] = (half == (fr >> 3) && e == (fr & 7)) ? (half_t)1.f : (half_t)0.f;
    const half8 fhot1 = frame_hot1<NB>(fr, half);
    const int klim = F - 4 * half;
    const float c2 = p.scale * 1.4426950408889634f;

#pragma unroll 1
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int pix = tile * 4 * PPW + wid * PPW + pp;
        const bool mok = pix < p.npix && (!MASKED || fr < F);
        const int b = pix / p.HW, pl = pix - b * p.HW;
        const int64_t m = ((int64_t)b * F + fr) * p.HW + pl;
        const unsigned xoff = mok ? (unsigned)((m * p.ldx + 8 * half) * 2) : OOB_OFFSET;
        const unsigned ooff = mok ? (unsigned)((m * p.ldo + 8 * half) * 2) : OOB_OFFSET;
        half8 xn[KS];
        load_rows<KS, true>(xn, rX, xoff, p.eps);

#pragma unroll 1
        for (int G = 0; G < 4; ++G) {
            half8 qs[10], ks[10];
            half8 PB[2][2];
            float invl[2];
            floatx16 acc0, acc1;
            const uint4v nores[2] = {};
            half8 fb[2][8];

            auto scores = [&]() {
                floatx16 S[2];
                zero16(S[0]); zero16(S[1]);
                static_for<5>([&](auto st_) {   // heads interleaved: two independent MFMA chains
                    constexpr int st = decltype(st_)::value;
                    S[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ks[st], qs[st], S[0], 0, 0, 0);
                    S[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ks[5 + st], qs[5 + st], S[1], 0, 0, 0);
                });
#pragma unroll
                for (int h = 0; h < 2; ++h) tattn_softmax<FP, MASKED>(S[h], pp, klim, c2, PB[h], invl[h]);
            };
            // O^T of local tile tl from its packed V tile -> memory (channels 160 G + 32 tl ..)
            auto pv_tile = [&](auto tl_, const floatx16& accV) {
                constexpr int tl = decltype(tl_)::value;
                constexpr int ha = (32 * tl) / 80, hb = (32 * tl + 31) / 80;
                half8 v0, v1;
                pack_tile(accV, v0, v1);
                floatx16 Oa, Ob;
                zero16(Oa);
                Oa = __builtin_amdgcn_mfma_f32_32x32x16_f16(v0, PB[ha][0], Oa, 0, 0, 0);
                Oa = __builtin_amdgcn_mfma_f32_32x32x16_f16(v1, PB[ha][1], Oa, 0, 0, 0);
                if (hb != ha) {
                    zero16(Ob);
                    Ob = __builtin_amdgcn_mfma_f32_32x32x16_f16(v0, PB[hb][0], Ob, 0, 0, 0);
                    Ob = __builtin_amdgcn_mfma_f32_32x32x16_f16(v1, PB[hb][1], Ob, 0, 0, 0);
                }
                floatx16 o;
#pragma unroll
                for (int qd = 0; qd < 4; ++qd) {
                    const int h = (32 * tl + 8 * qd) / 80;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[4 * qd + e] = (h == ha ? Oa[4 * qd + e] : Ob[4 * qd + e]) * invl[h];
                }
                store_tile<false>(o, nores, rO, ooff, (160 * G + 32 * tl) * 2);
            };

            auto consume_group = [&](auto g_) {
                constexpr int g = decltype(g_)::value;
                static_for<8>([&](auto i_) {
                    constexpr int i = decltype(i_)::value, f = g * 8 + i;
                    constexpr TbOp op = tb_op<NB>(f);
                    const half8 a = fb[g & 1][i];
                    if constexpr (op.kind == 1 || op.kind == 2) {          // q / k tile of the group: A = weights, B = tokens
                        const half8 bop = op.s < KS ? xn[op.s < KS ? op.s : 0] : op.s == KS ? fhot : fhot1;
                        if constexpr (op.kind == 1) {
                            if (op.s == 0) zero16(acc0);
                            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc0, 0, 0, 0);
                        } else {
                            if (op.s == 0) zero16(acc1);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc1, 0, 0, 0);
                            if constexpr (op.s == SC::KSB - 1) {
                                pack_tile(acc0, qs[2 * op.t], qs[2 * op.t + 1]);
                                pack_tile(acc1, ks[2 * op.t], ks[2 * op.t + 1]);
                                if constexpr (op.t == 4) scores();
                            }
                        }
                    } else if constexpr (op.kind == 3) {                    // v tile, operands swapped: [token][channel]
                        const half8 aop = op.s < KS ? xn[op.s < KS ? op.s : 0] : op.s == KS ? fhot : fhot1;
                        constexpr bool second = op.t == 1 || op.t == 3;
                        if constexpr (second) {
                            if (op.s == 0) zero16(acc1);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(aop, a, acc1, 0, 0, 0);
                            if constexpr (op.s == SC::KSB - 1) { pv_tile(ic<op.t - 1>{}, acc0); pv_tile(ic<op.t>{}, acc1); }
                        } else {
                            if (op.s == 0) zero16(acc0);
                            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(aop, a, acc0, 0, 0, 0);
                            if constexpr (op.s == SC::KSB - 1 && op.t == 4) pv_tile(ic<4>{}, acc0);
                        }
                    }
                    if (i == 3) ring.template refill<g % R::GPS, 0>();
                    if (i == 7) ring.template refill<g % R::GPS, 1>();
                });
                tattn_group_pipeline();
            };
            constexpr int NG = SC::GROUP_FR / 8;   // 78 (FP = 16) / 80 (FP = 32) groups per head group: even, so a head group starts on a slot
            ring.template read_group<0>(fb[0]);
            static_for<NG - 1>([&](auto g_) {
                constexpr int g = decltype(g_)::value;
                ring.template read_group<g + 1>(fb[(g + 1) & 1]);
                consume_group(ic<g>{});
            });
            consume_group(ic<NG - 1>{});
        }
    }
    wait_vmcnt<0>();
}

}  // namespace

extern "C" int insv2v_tattn_attn(const insv2v_tattn_desc* dp, insv2v_stream_t stream) {
    static const void* const kernels[3] = {(const void*)tattn640_kernel<16, false>, (const void*)tattn640_kernel<16, true>, (const void*)tattn640_kernel<32, true>};
    static bool attr_set[3] = {};
    return launch_tattn(dp, 640, kernels, attr_set, stream);
}

extern "C" int64_t insv2v_tattn_attn_stream_elems(int32_t C, int32_t heads, int32_t frames) {
    if (C != 640 || heads != TA_H || frames < 1 || frames > 32) return 0;
    return (int64_t)4 * (frames <= TA_F ? TbSched<1>::GROUP_FR : TbSched<2>::GROUP_FR) * 512;
}
