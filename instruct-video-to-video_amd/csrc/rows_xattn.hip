// Fused text cross-attention: insv2v_xattn_fused (C = 320) and insv2v_xattn_attn (C = 640); the register-resident scheme: rows_common.h
#include "rows_common.h"
#include <algorithm>

namespace {
// ===================================================================================================== cross-attention block
// insv2v_xattn_fused: the text cross-attention sub-block of BasicTransformerBlock (attention.py:249-257: norm2 -> attn2 + residual) at
// C = 320, 8 heads x 40, up to 96 text tokens, as ONE register-resident launch:
//     out = x + Wo . Attn( LayerNorm(x) Wq^T + Wq beta ;  K_b, V_b ) + bo          (b = the sample of the token row)
// The text K / V of a sample are only 2 x 77 x 320 halfs and loop-invariant over the sampling loop, so they are a second WEIGHT STREAM:
// insv2v/fused.py pack_xattn_kv lays them out per sample as MFMA A fragments, masked per head, in the order consumed here, and the
// ring pulls them through LDS between the shared q-projection and output-projection weights.  A 128-row tile lies inside one sample for
// every rows_per_sample - the segmented row schedule, XattnTile below.
//   * q tiles ([32 channels] x [32 tokens], C layout) packed to fp16 are the B fragments of S^T = K_h . Q_h^T: a head is 40 channels = 5
//     octets = two full k-steps + one half k-step whose other octet is ZERO IN THE K FRAGMENT (no masking in the kernel);
//   * S^T is [96 keys] x [32 tokens] per head (3 accumulator tiles): softmax over the keys = in-lane over 48 values + one exchange with the
//     other lane half; keys >= ctx_len get an additive -1e30; the NORMALISED probabilities packed to fp16 are the B fragments (k = keys)
//     of O^T += V_h^T . P^T, with V_h^T fragments zero outside the head's channels so the group's 5 output tiles simply accumulate;
//   * O^T tiles packed are the B fragments of the output projection; residual and store as in the row Linears.
// Stream per tile, 39 slots of 16 fragments: [Q: 5 tile pairs x 21 k-steps, pad 14] [per sample: 8 heads x (9 K + 12 V), pad 8]
// [OUT: 5 tile pairs x 21, pad 14].  The per-sample slots are requested 8 slots ahead like all others, which is still inside the tile.
struct XattnArgs {
    const half_t* x;
    half_t* out;
    const half_t* wstream;
    const half_t* kvstream;
    int64_t ldx, ldo;
    int M, rows_per_sample, ctx_len;
    float eps, scale;
    const half_t* pre_res;   // PRE: residual of the leading Linear (x is then the self-attention output), row stride ld_pre
    int64_t ld_pre;
    int tiles_per_sample, ntiles;   // ceil(rows_per_sample / 128), samples * tiles_per_sample (xattn_args)
};
// The segmented row schedule of both text kernels: every sample gets ceil(rows_per_sample / 128) tiles of its own, so a tile never straddles
// two samples' K / V streams whatever rows_per_sample is.  Tile t = (sample t / tiles_per_sample, unit t % tiles_per_sample) covers the real
// rows sample * rows_per_sample + unit * 128 .. + 127; the overhang of a sample's last tile (rows at or beyond rows_per_sample) reads zeros
// and is never stored (OOB offsets, as rows beyond M always were).  One wave-uniform division per tile, none per lane; with
// rows_per_sample % 128 == 0 this is the plain tiling of the M rows.
struct XattnTile {
    int sample;   // wave-uniform
    int m;        // this lane's token row
    bool mok;     // ... is a real row of the sample
    __device__ __forceinline__ XattnTile(const XattnArgs& p, int tile, int wid, int tok) {
        sample = __builtin_amdgcn_readfirstlane(tile / p.tiles_per_sample);
        const int ml = (tile - sample * p.tiles_per_sample) * 128 + wid * 32 + tok;
        m = sample * p.rows_per_sample + ml;
        mok = ml < p.rows_per_sample;
    }
};
constexpr int XA_Q_FR = 224, XA_KV_FR = 176, XA_O_FR = 224, XA_TOTAL = XA_Q_FR + XA_KV_FR + XA_O_FR;
constexpr int XA_QS = XA_Q_FR / 16, XA_KVS = XA_KV_FR / 16;
// PRE: the out-projection of the preceding self-attention (attention.py:244-247: hidden = attn1(norm1(hidden)) + hidden) rides in front:
// x1 = Wo1 . a + bo1 + h never leaves the registers - its finished tiles (finish_tile) ARE the natural-order fragments the LayerNorm and the
// q projection read, and the raw copy is the residual of the block's output.  Stream: + [output tiles in pairs x 21: 210][pad 14] = 14 slots.
constexpr int XA_PRE_FR = 224;
struct XaOp { int kind, a, b, c; };   // 0 pad | 1 Q (tile a, k-step b) | 2 K (head a of 8, key tile b, step c) | 3 V (head a, tile select b, key k-step c) | 4 OUT (tile a, k-step b) | 5 PRE (tile a, k-step b)
template <bool PRE>
constexpr XaOp xa_op(int f) {
    if (PRE) {
        if (f < 210) return {5, 2 * (f / 42) + (f % 42 & 1), (f % 42) >> 1, 0};
        if (f < XA_PRE_FR) return {0, 0, 0, 0};
        f -= XA_PRE_FR;
    }
    if (f < XA_Q_FR) {
        if (f < 210) return {1, 2 * (f / 42) + (f % 42 & 1), (f % 42) >> 1, 0};
        return {0, 0, 0, 0};
    }
    f -= XA_Q_FR;
    if (f < XA_KV_FR) {
        if (f >= 168) return {0, 0, 0, 0};
        const int gh = f / 21, r = f % 21;
        if (r < 9) return {2, gh, r % 3, r / 3};
        return {3, gh, (r - 9) & 1, (r - 9) >> 1};
    }
    f -= XA_KV_FR;
    if (f < 210) return {4, 2 * (f / 42) + (f % 42 & 1), (f % 42) >> 1, 0};
    return {0, 0, 0, 0};
}
// group-local k-step (16 channels of the 160-channel head group) of step st of head h: see tattn_fused_kernel::scores
constexpr int xa_kstep(int h, int st) {
    const int lo = 5 * h;
    if (st < 2) return (lo & 1) ? (lo + 1) / 2 + st : lo / 2 + st;
    return ((lo & 1) ? lo : lo + 4) >> 1;
}

// The ring of both text kernels: Ring<16, 9> with TWO sources - the shared weights (rW) and the tile's per-sample K / V stream (rKV, from
// byte kv_soff on).  The LDS side (state, advance_lds, acquire, read_group) is Ring's; its linear-source fields iss_soff / pass_bytes stay
// unused.  A kernel's ring adds only how a compile-time stream slot maps to a source and an offset (piece), and requests NS - 1 slots
// ahead in init.
struct KvRing : Ring<16, 9> {
    srd_t rKV;
    int kv_soff;
    __device__ __forceinline__ void init_kv(char* smem_, const void* w, const void* kvs, int wid, int lane) {
        smem = smem_;
        rW = make_srd(w);
        rKV = make_srd(kvs);
        lane16 = (unsigned)(lane * 16);
        wave_off = wid * PPS * 1024;
        iss_lds = 0; kv_soff = 0;
        rd_off = (NS - 1) * SLOT_B;
        rd = smem_;
    }
    // piece i (1 KiB) of this wave's share of the slot at byte `off` of the K / V stream (KV) or of the shared weights
    template <bool KV>
    __device__ __forceinline__ void request(int off, int i) {
        if (KV) dma16(rKV, lane16, kv_soff + off + wave_off + i * 1024, smem + iss_lds + wave_off + i * 1024);
        else dma16(rW, lane16, off + wave_off + i * 1024, smem + iss_lds + wave_off + i * 1024);
    }
};
// Softmax over the 96 keys of one head for the lane's query: the additive mask on the third key tile, maximum and sum = 48 in-lane values +
// one exchange with the other lane half, the NORMALISED probabilities packed as the key k-steps 0 .. 5 of O^T += V^T . P^T.  A function
// object bound to the kernel's S, kmask, c2 and P, declared per tile where the per-kernel lambda it replaces stood: in this form the
// instruction streams of the three text kernels stay exactly as they were (as a plain function hipcc swaps the operands of one v_add_f32
// per head).
struct XattnSoftmax {
    floatx16 (&S)[3];
    const float (&kmask)[16];
    const float& c2;
    half8 (&P)[6];
    __device__ void operator()() const {
#pragma unroll
        for (int r = 0; r < 16; ++r) S[2][r] += kmask[r];
        float mx = S[0][0];
#pragma unroll
        for (int kt = 0; kt < 3; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) mx = fmaxf(mx, S[kt][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mc = -mx * c2;
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < 3; ++kt)
#pragma unroll
            for (int r = 0; r < 16; ++r) { const float e = __builtin_amdgcn_exp2f(fmaf(S[kt][r], c2, mc)); S[kt][r] = e; l += e; }
        l += __shfl_xor(l, 32, 64);
        const float inv = 1.f / l;
#pragma unroll
        for (int kt = 0; kt < 3; ++kt) {
#pragma unroll
            for (int r = 0; r < 16; ++r) S[kt][r] *= inv;
            pack_tile(S[kt], P[2 * kt], P[2 * kt + 1]);
        }
    }
};

// C = 320: the source of a stream slot is static - the shared weights, or the tile's per-sample K / V behind the q section
template <int NPRE>   // slots of a leading shared-weight section in front of the q section
struct XRing : KvRing {
    template <int SLOT>
    __device__ __forceinline__ void piece(int i) {
        constexpr bool kv = SLOT >= NPRE + XA_QS && SLOT < NPRE + XA_QS + XA_KVS;
        request<kv>((kv ? SLOT - NPRE - XA_QS : (SLOT < NPRE + XA_QS ? SLOT : SLOT - XA_KVS)) * SLOT_B, i);
    }
    __device__ __forceinline__ void init(char* smem_, const void* w, const void* kvs, int wid, int lane) {
        init_kv(smem_, w, kvs, wid, lane);
        static_for<NS - 1>([&](auto s_) {
#pragma unroll
            for (int i = 0; i < PPS; ++i) piece<decltype(s_)::value>(i);
            advance_lds();
        });
    }
    template <int SLOT>
    __device__ __forceinline__ void refill(int ph, int which) {
        piece<SLOT>(2 * ph + which);
        if (which == 1 && ph == GPS - 1) advance_lds();
    }
};

template <bool PRE>
__global__ __launch_bounds__(256, 1) void xattn_fused_kernel(XattnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NPRE = PRE ? XA_PRE_FR / 16 : 0, TOTAL = XA_TOTAL + (PRE ? XA_PRE_FR : 0), SLOTS = TOTAL / 16;
    typedef XRing<NPRE> RingT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tok = lane & 31, half = lane >> 5;
    const int ntiles = p.ntiles;
    const srd_t rX = make_srd(p.x), rO = make_srd(p.out), rH = make_srd(PRE ? (const void*)p.pre_res : (const void*)p.x);
    RingT ring;
    ring.init(smem, p.wstream, p.kvstream, wid, lane);

    const half8 ones = bias_ones(half);
    const float c2 = p.scale * 1.4426950408889634f;
    // additive key mask of the third key tile (keys 64 + (r & 3) + 8 (r >> 2) + 4 half): ctx_len is in (64, 96]
    float kmask[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) kmask[r] = (64 + (r & 3) + 8 * (r >> 2) + 4 * half) < p.ctx_len ? 0.f : -1.0e30f;

#pragma unroll 1
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const XattnTile rt(p, tile, wid, tok);
        const int m = rt.m;
        const bool mok = rt.mok;
        const unsigned xoff = mok ? (unsigned)(((int64_t)m * p.ldx + 8 * half) * 2) : OOB_OFFSET;
        const unsigned ooff = mok ? (unsigned)(((int64_t)m * p.ldo + 8 * half) * 2) : OOB_OFFSET;
        ring.kv_soff = rt.sample * (XA_KV_FR * 1024);
        const unsigned hoff = (PRE && mok) ? (unsigned)(((int64_t)m * p.ld_pre + 8 * half) * 2) : OOB_OFFSET;
        half8 xn[KS1];                     // PRE: first the self-attention output (operand of the leading Linear), then LayerNorm(x1)
        half8 x1[PRE ? KS1 : 1];           // PRE: x1 = leading Linear + residual, raw: the residual of the block's output
        load_rows<KS1, !PRE>(xn, rX, xoff, p.eps);

        half8 qs[KS1];                     // q of all 10 channel tiles, packed per k-step
        half8 afr[KS1];                    // attention output, packed: the B fragments of the output projection
        half8 P[6];                        // normalised probabilities of the current head: key k-steps 0..5
        floatx16 S[3], O[5];
        floatx16 acc0, acc1;
        uint4v resv[2][2];
        half8 fb[2][8];

        XattnSoftmax softmax{S, kmask, c2, P};

        auto consume_group = [&](auto g_) {
            constexpr int g = decltype(g_)::value;
            constexpr int islot = (g / RingT::GPS + RingT::NS - 1) % SLOTS;   // the stream slot whose pieces this group requests
            static_for<8>([&](auto i_) {
                constexpr int i = decltype(i_)::value, f = g * 8 + i;
                constexpr XaOp op = xa_op<PRE>(f);
                const half8 a = fb[g & 1][i];
                if constexpr (op.kind == 5) {                           // PRE: x1 = Wo1 . a + bo1 + h, tiles in pairs, finished into fragments
                    const half8 bop = op.b < KS1 ? xn[op.b < KS1 ? op.b : 0] : ones;
                    if constexpr ((op.a & 1) == 0) {
                        if (op.b == 0) { zero16(acc0); load_res_tile<true>(resv[0], rH, hoff, op.a * 64); load_res_tile<true>(resv[1], rH, hoff, op.a * 64 + 64); }
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc0, 0, 0, 0);
                    } else {
                        if (op.b == 0) zero16(acc1);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc1, 0, 0, 0);
                        if constexpr (op.b == KS1) {
                            half8 t0[2], t1[2];
                            finish_tile<true>(acc0, resv[0], t0);
                            finish_tile<true>(acc1, resv[1], t1);
                            x1[PRE ? 2 * (op.a - 1) : 0] = t0[0]; x1[PRE ? 2 * (op.a - 1) + 1 : 0] = t0[1];
                            x1[PRE ? 2 * op.a : 0] = t1[0]; x1[PRE ? 2 * op.a + 1 : 0] = t1[1];
                            if constexpr (op.a == 9) {              // all of x1 is there: it replaces the operand, normalised
#pragma unroll
                                for (int k = 0; k < KS1; ++k) xn[k] = x1[PRE ? k : 0];
                                layernorm_frags<KS1>(xn, p.eps);
                            }
                        }
                    }
                } else if constexpr (op.kind == 1) {                           // q projection, tiles in pairs
                    const half8 bop = op.b < KS1 ? xn[op.b < KS1 ? op.b : 0] : ones;
                    if constexpr ((op.a & 1) == 0) {
                        if (op.b == 0) zero16(acc0);
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc0, 0, 0, 0);
                    } else {
                        if (op.b == 0) zero16(acc1);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc1, 0, 0, 0);
                        if constexpr (op.b == KS1) {
                            pack_tile(acc0, qs[2 * (op.a - 1)], qs[2 * (op.a - 1) + 1]);
                            pack_tile(acc1, qs[2 * op.a], qs[2 * op.a + 1]);
                        }
                    }
                } else if constexpr (op.kind == 2) {                    // scores of head op.a: S^T[key tile op.b] += K . Q^T
                    constexpr int G = op.a >> 2, h = op.a & 3, kst = 10 * G + xa_kstep(h, op.c);
                    if (op.c == 0) zero16(S[op.b]);
                    S[op.b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qs[kst], S[op.b], 0, 0, 0);
                    if constexpr (op.c == 2 && op.b == 2) softmax();
                } else if constexpr (op.kind == 3) {                    // O^T[tile] += V_h^T . P^T
                    constexpr int G = op.a >> 2, h = op.a & 3, t = (40 * h) / 32 + op.b;
                    if constexpr (h == 0 && op.b == 0 && op.c == 0) {
#pragma unroll
                        for (int q = 0; q < 5; ++q) zero16(O[q]);
                    }
                    O[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, P[op.c], O[t], 0, 0, 0);
                    if constexpr (h == 3 && op.b == 1 && op.c == 5) {
#pragma unroll
                        for (int q = 0; q < 5; ++q) pack_tile(O[q], afr[2 * (5 * G + q)], afr[2 * (5 * G + q) + 1]);
                    }
                } else if constexpr (op.kind == 4) {                    // output projection + residual, tiles in pairs
                    const half8 bop = op.b < KS1 ? afr[op.b < KS1 ? op.b : 0] : ones;
                    if constexpr ((op.a & 1) == 0) {
                        if (op.b == 0) {
                            zero16(acc0);
                            if (PRE) {   // the residual x1 never left the registers: its fragments are the 16-byte chunks store_tile adds
#pragma unroll
                                for (int j = 0; j < 2; ++j) {
                                    resv[0][j] = __builtin_bit_cast(uint4v, x1[PRE ? 2 * op.a + j : 0]);
                                    resv[1][j] = __builtin_bit_cast(uint4v, x1[PRE ? 2 * op.a + 2 + j : 0]);
                                }
                            } else {
                                load_res_tile<true>(resv[0], rX, xoff, op.a * 64); load_res_tile<true>(resv[1], rX, xoff, op.a * 64 + 64);
                            }
                        }
                        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc0, 0, 0, 0);
                    } else {
                        if (op.b == 0) zero16(acc1);
                        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc1, 0, 0, 0);
                        if constexpr (op.b == KS1) {
                            store_tile<true>(acc0, resv[0], rO, ooff, (op.a - 1) * 64);
                            store_tile<true>(acc1, resv[1], rO, ooff, op.a * 64);
                        }
                    }
                }
                if (i == 3) ring.template refill<islot>(g % RingT::GPS, 0);
                if (i == 7) ring.template refill<islot>(g % RingT::GPS, 1);
            });
        };
        constexpr int NG = TOTAL / 8;   // 78 (PRE: 106) groups per tile
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

// Both launchers: validation and the argument block; kv_fr = fragments of one sample's K / V stream
// (x, out and pre_residual may each exceed the 2 GiB window: launch_xattn runs ranges of whole samples; the K / V streams of all samples
// stay inside one window)
static int xattn_args(const insv2v_xattn_desc* dp, int C, int kv_fr, XattnArgs& a) {
    if (!one_device()) return INSV2V_EINVAL;
    if (!dp) return INSV2V_EINVAL;
    const insv2v_xattn_desc& d = *dp;
    if (!d.x || !d.out || !d.wstream || !d.kvstream || d.M <= 0 || d.rows_per_sample <= 0) return INSV2V_EINVAL;
    if (d.C != C || d.heads != 8 || d.ctx_len <= 64 || d.ctx_len > 96) return INSV2V_EUNSUPPORTED;
    if (d.M % d.rows_per_sample) return INSV2V_EUNSUPPORTED;   // whole samples: each gets its own 128-row tiles (XattnTile)
    if ((d.ldx & 7) || (d.ldo & 7) || ((uintptr_t)d.x & 15) || ((uintptr_t)d.out & 15) || ((uintptr_t)d.wstream & 15) || ((uintptr_t)d.kvstream & 15)) return INSV2V_EINVAL;
    const int64_t lim = (int64_t)1 << 31;
    if ((int64_t)(d.M / d.rows_per_sample) * kv_fr * 1024 >= lim) return INSV2V_EUNSUPPORTED;
    a = {(const half_t*)d.x, (half_t*)d.out, (const half_t*)d.wstream, (const half_t*)d.kvstream, d.ldx, d.ldo, d.M, d.rows_per_sample,
         d.ctx_len, d.eps, d.scale, nullptr, 0, 0, 0};
    a.tiles_per_sample = (d.rows_per_sample + 127) / 128;
    a.ntiles = 0;   // (per range: launch_xattn)
    return 0;
}
// ranges of whole samples, one launch each (launch_unit_ranges): the row operands and the samples' K / V streams advance together
static int launch_xattn(const void* kernel, bool& attr_set, const XattnArgs& a, int kv_fr, insv2v_stream_t stream) {
    const int64_t ld = std::max(std::max(a.ldx, a.ldo), a.pre_res ? a.ld_pre : (int64_t)0);
    return launch_unit_ranges(a.M / a.rows_per_sample, (int64_t)a.rows_per_sample * ld * 2, [&](int64_t s0, int64_t ns) {
        if (ns * a.tiles_per_sample * 128 > 0x7fffffff) return (int)INSV2V_EUNSUPPORTED;
        XattnArgs r = a;
        const int64_t m0 = s0 * a.rows_per_sample;
        r.x += m0 * a.ldx; r.out += m0 * a.ldo;
        if (a.pre_res) r.pre_res += m0 * a.ld_pre;
        r.kvstream += s0 * kv_fr * 512;
        r.M = (int)(ns * a.rows_per_sample);
        r.ntiles = (int)(ns * a.tiles_per_sample);
        return launch_rows(kernel, attr_set, KvRing::NS * KvRing::SLOT_B, r, r.ntiles * 128, as_stream(stream));
    });
}

extern "C" int insv2v_xattn_fused(const insv2v_xattn_desc* dp, insv2v_stream_t stream) {
    XattnArgs a;
    if (const int st = xattn_args(dp, FC, XA_KV_FR, a)) return st;
    const insv2v_xattn_desc& d = *dp;
    static bool attr_set = false;
    if (d.pre_residual) {
        if ((d.ld_pre & 7) || ((uintptr_t)d.pre_residual & 15)) return INSV2V_EINVAL;
        a.pre_res = (const half_t*)d.pre_residual;
        a.ld_pre = d.ld_pre;
        static bool pre_attr = false;
        return launch_xattn((const void*)xattn_fused_kernel<true>, pre_attr, a, XA_KV_FR, stream);
    }
    return launch_xattn((const void*)xattn_fused_kernel<false>, attr_set, a, XA_KV_FR, stream);
}

// fp16 elements of the shared weight stream (q + output projections) and of ONE sample's K / V stream; 0 if unsupported
extern "C" int64_t insv2v_xattn_stream_elems(int32_t C, int32_t heads, int32_t per_sample_kv) {   // per_sample_kv: 0 = shared weights, 1 = one sample's K / V, 2 = shared weights with the leading Linear
    if (C != FC || heads != 8) return 0;
    return (int64_t)(per_sample_kv == 1 ? XA_KV_FR : XA_Q_FR + XA_O_FR + (per_sample_kv == 2 ? XA_PRE_FR : 0)) * 512;
}

namespace {
// ===================================================================================================== cross-attention, C = 640
// insv2v_xattn_attn: LayerNorm -> q -> attention over the sample's text tokens at C = 640 (8 heads x 80), WITHOUT the output projection
// (same register argument as tattn640_kernel): the attention output [rows, 640] goes to memory, to_out + residual follow as insv2v_rowlin.
// A head = 5 whole k-steps of a 160-channel group; per group the ring pulls 13 slots of q weights (5 tiles x 41 k-steps) and 5 slots of the
// sample's K / V fragments (2 heads x (15 K + 18 V)); the group loop is a run-time loop around one unrolled group body.
constexpr int XB_Q_FR = 208, XB_KV_FR = 80, XB_GROUP_FR = XB_Q_FR + XB_KV_FR, XB_QS = XB_Q_FR / 16, XB_KVS = XB_KV_FR / 16, XB_SLOTS = XB_GROUP_FR / 16;
struct XbOp { int kind, a, b, c; };   // 0 pad | 1 Q (tile a, k-step b) | 2 K (head a, key tile b, step c) | 3 V (head a, tile select b, key k-step c)
constexpr XbOp xb_op(int f) {
    if (f < XB_Q_FR) {
        if (f < 164) return {1, 2 * (f / 82) + (f % 82 & 1), (f % 82) >> 1, 0};
        if (f < 205) return {1, 4, f - 164, 0};
        return {0, 0, 0, 0};
    }
    const int r = f - XB_Q_FR;
    if (r >= 66) return {0, 0, 0, 0};
    const int h = r / 33, q = r % 33;
    if (q < 15) return {2, h, q % 3, q / 3};
    return {3, h, (q - 15) % 3, (q - 15) / 3};
}

// C = 640: the source of a slot is resolved from a static slot of the group + the run-time group Gi: its q weights or the sample's K / V
struct XbRing : KvRing {
    template <int SLOT>   // SLOT in [0, XB_SLOTS): slot of group Gi
    __device__ __forceinline__ void piece(int i, int Gi) {
        constexpr bool kv = SLOT >= XB_QS;
        request<kv>((kv ? Gi * XB_KVS + SLOT - XB_QS : Gi * XB_QS + SLOT) * SLOT_B, i);
    }
    __device__ __forceinline__ void init(char* smem_, const void* w, const void* kvs, int wid, int lane) {
        init_kv(smem_, w, kvs, wid, lane);
        static_for<NS - 1>([&](auto s_) {   // slots 0 .. 7 of group 0: q weights
#pragma unroll
            for (int i = 0; i < PPS; ++i) piece<decltype(s_)::value>(i, 0);
            advance_lds();
        });
    }
};

__global__ __launch_bounds__(256, 1) void xattn640_kernel(XattnArgs p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int KS = 40;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tok = lane & 31, half = lane >> 5;
    const int ntiles = p.ntiles;
    const srd_t rX = make_srd(p.x), rO = make_srd(p.out);
    XbRing ring;
    ring.init(smem, p.wstream, p.kvstream, wid, lane);

    const half8 ones = bias_ones(half);
    const float c2 = p.scale * 1.4426950408889634f;
    float kmask[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) kmask[r] = (64 + (r & 3) + 8 * (r >> 2) + 4 * half) < p.ctx_len ? 0.f : -1.0e30f;

#pragma unroll 1
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const XattnTile rt(p, tile, wid, tok);
        const int m = rt.m;
        const bool mok = rt.mok;
        const unsigned xoff = mok ? (unsigned)(((int64_t)m * p.ldx + 8 * half) * 2) : OOB_OFFSET;
        const unsigned ooff = mok ? (unsigned)(((int64_t)m * p.ldo + 8 * half) * 2) : OOB_OFFSET;
        ring.kv_soff = rt.sample * (4 * XB_KV_FR * 1024);
        half8 xn[KS];
        load_rows<KS, true>(xn, rX, xoff, p.eps);

#pragma unroll 1
        for (int G = 0; G < 4; ++G) {
            half8 qs[10];
            half8 P[6];
            floatx16 S[3], O[5];
            floatx16 acc0, acc1;
            const uint4v nores[2] = {};
            half8 fb[2][8];

            XattnSoftmax softmax{S, kmask, c2, P};

            auto consume_group = [&](auto g_) {
                constexpr int g = decltype(g_)::value;
                constexpr int ahead = g / XbRing::GPS + XbRing::NS - 1, islot = ahead % XB_SLOTS;   // slot requested by this group: of group G or G + 1
                const int Gi = (G + (ahead >= XB_SLOTS ? 1 : 0)) & 3;                               // (wraps into the next tile's group 0: q weights only)
                static_for<8>([&](auto i_) {
                    constexpr int i = decltype(i_)::value, f = g * 8 + i;
                    constexpr XbOp op = xb_op(f);
                    const half8 a = fb[g & 1][i];
                    if constexpr (op.kind == 1) {                           // q projection of the group's 5 tiles: pairs (0,1), (2,3), then 4
                        const half8 bop = op.b < KS ? xn[op.b < KS ? op.b : 0] : ones;
                        if constexpr ((op.a & 1) == 0) {
                            if (op.b == 0) zero16(acc0);
                            acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc0, 0, 0, 0);
                            if constexpr (op.a == 4 && op.b == KS) pack_tile(acc0, qs[8], qs[9]);
                        } else {
                            if (op.b == 0) zero16(acc1);
                            acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bop, acc1, 0, 0, 0);
                            if constexpr (op.b == KS) {
                                pack_tile(acc0, qs[2 * (op.a - 1)], qs[2 * (op.a - 1) + 1]);
                                pack_tile(acc1, qs[2 * op.a], qs[2 * op.a + 1]);
                            }
                        }
                    } else if constexpr (op.kind == 2) {                    // scores of head op.a: S^T[key tile op.b] += K . Q^T over its 5 k-steps
                        if (op.c == 0) zero16(S[op.b]);
                        S[op.b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qs[5 * op.a + op.c], S[op.b], 0, 0, 0);
                        if constexpr (op.c == 4 && op.b == 2) softmax();
                    } else if constexpr (op.kind == 3) {                    // O^T[tile] += V_h^T . P^T; head 0: tiles 0-2, head 1: tiles 2-4
                        constexpr int t = 2 * op.a + op.b;
                        if constexpr (op.a == 0 && op.b == 0 && op.c == 0) {
#pragma unroll
                            for (int q = 0; q < 5; ++q) zero16(O[q]);
                        }
                        O[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, P[op.c], O[t], 0, 0, 0);
                        if constexpr (op.a == 1 && op.b == 2 && op.c == 5) {
#pragma unroll
                            for (int q = 0; q < 5; ++q) store_tile<false>(O[q], nores, rO, ooff, (160 * G + 32 * q) * 2);
                        }
                    }
                    if (i == 3) { ring.template piece<islot>(2 * (g % XbRing::GPS), Gi); }
                    if (i == 7) { ring.template piece<islot>(2 * (g % XbRing::GPS) + 1, Gi); if (g % XbRing::GPS == XbRing::GPS - 1) ring.advance_lds(); }
                });
            };
            constexpr int NG = XB_GROUP_FR / 8;   // 36 groups per head group
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

extern "C" int insv2v_xattn_attn(const insv2v_xattn_desc* dp, insv2v_stream_t stream) {
    XattnArgs a;
    if (const int st = xattn_args(dp, 640, 4 * XB_KV_FR, a)) return st;
    static bool attr_set = false;
    return launch_xattn((const void*)xattn640_kernel, attr_set, a, 4 * XB_KV_FR, stream);
}

// fp16 elements of the q weight stream / of ONE sample's K / V stream of insv2v_xattn_attn; 0 if unsupported
extern "C" int64_t insv2v_xattn_attn_stream_elems(int32_t C, int32_t heads, int32_t per_sample_kv) {
    if (C != 640 || heads != 8) return 0;
    return (int64_t)4 * (per_sample_kv ? XB_KV_FR : XB_Q_FR) * 512;
}
