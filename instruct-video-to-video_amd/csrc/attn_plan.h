// The dispatch of insv2v_attention as a pure function: plan_attention(descriptor, switches, cus) -> insv2v_attention_plan_t.
// Host-only, no HIP call, no static, no environment read.  insv2v_attention validates through it, then launches what it says;
// insv2v_attention_plan returns it without touching a GPU.  The limits below are the kernels' own (attention.hip static_asserts them).
#pragma once
#include <stdint.h>
#include "../../include/insv2v_hip.h"

constexpr int ATTN_SHORT_MAXT = 512;            // attn_short_kernel<D, BIAS = true>: its launch bound (the bias fragments' register budget) = 8 heads
constexpr int ATTN_SHORT_MAX_HEADS = 16;        // one wave per head, <= 1024 threads
constexpr int ATTN_SHORT_ROWS = 16;             // queries and keys it holds (one MFMA block)
constexpr int ATTN_SHORT_VT_LD = 20;            // halfs per row of its transposed V slice
constexpr int ATTN_SHORT_LDS_MAX = 64 * 1024;   // the dynamic LDS a launch gets without asking for more
constexpr int ATTN_SINGLE_O_ALIGN = 16;         // attn_kernel<.., SINGLE>: bytes of its output stores (base, row, problem strides)
constexpr int ATTN_SINGLE_KVT = 96;             // its one key tile = its six waves' query rows
constexpr int ATTN_LDS_MAX = 160 * 1024;        // LDS of a CU: what hipFuncSetAttribute may raise a launch to
constexpr int64_t ATTN_WINDOW = 0x7fffffffLL;   // bytes a K / V buffer descriptor spans from the (problem, head) base (32-bit offsets)

// The A/B switches of the attention dispatch, read once (insv2v_attention_switches, attention.hip).  Defaults = the product.
struct attention_switches {
    int short_on = 1;    // INSV2V_ATTN_SHORT: the one-wave-per-head kernel for <= 16 rows (bias tables take it regardless)
    int fold = 1;        // INSV2V_ATTN_FOLD: the folded softmax at d = 40 / 80
    int single = 1;      // INSV2V_ATTN_SINGLE: the single-tile form at d = 160
    int rep = 1;         // INSV2V_ATTN_REP: ... serving the consecutive problems that share one K / V
    int short_wgs = 2;   // INSV2V_ATTN_SHORT_WGS: workgroups per CU of the persistent biased short kernel (0: one per problem)
};

constexpr bool attn_head_dim_ok(int d) { return d == 16 || d == 32 || d == 40 || d == 64 || d == 80 || d == 128 || d == 160; }
constexpr int attn_dp(int d) { return (d + 31) / 32 * 32; }                       // head dim padded to the MFMA K granularity
constexpr int attn_kvt(int nw) { return nw >= 4 ? 64 : 32; }                      // keys per tile of the generic forms
// attn_kernel's LDS: NBUF x (K tile [KVT][DP + 8] + V^T tile [DP][KVT + 4]) halfs
constexpr int64_t attn_lds_bytes(int d, int kvt, bool single) { return (int64_t)(single ? 1 : 2) * (kvt * (attn_dp(d) + 8) + attn_dp(d) * (kvt + 4)) * 2; }
constexpr int64_t attn_short_lds_bytes(int heads, int d) { return (int64_t)heads * ((d + 15) / 16) * 16 * ATTN_SHORT_VT_LD * 2; }
// (rows * rs + d) * 2 <= ATTN_WINDOW, without forming the product (any int64 stride)
constexpr bool attn_rows_fit(int64_t rows, int64_t rs, int d) { return rs <= (ATTN_WINDOW / 2 - d) / rows; }

static inline insv2v_attention_plan_t plan_attention(const insv2v_attention_desc& din, const attention_switches& sw, int cus) {
    insv2v_attention_plan_t p = {};
    p.family = INSV2V_ATTN_PLAN_NONE;
    p.rc = INSV2V_EINVAL;
    insv2v_attention_desc d = din;
    if (!d.q || !d.k || !d.v || !d.o) return p;
    if (d.head_dim <= 0 || (d.head_dim & 7) || (d.head_dim > 160 && d.head_dim != 512)) return p;
    if (d.seq_q <= 0 || d.seq_k <= 0 || d.batch <= 0 || d.heads <= 0) return p;
    if ((d.q_rs & 7) || (d.k_rs & 7) || (d.v_rs & 7) || (d.o_rs & 3)) return p;
    if (d.q_inner <= 0) d.q_inner = 1;
    if (d.kv_inner <= 0) d.kv_inner = 1;
    if (d.o_inner <= 0) d.o_inner = 1;
    const bool biased = d.q_bias || d.k_bias || d.v_bias;
    if (biased && (!d.q_bias || !d.k_bias || !d.v_bias || (d.bias_rs & 7) || ((uintptr_t)d.q_bias & 15) || ((uintptr_t)d.k_bias & 15) || ((uintptr_t)d.v_bias & 15)))
        return p;
    p.rc = INSV2V_EUNSUPPORTED;
    // every K / V tile load is a 32-bit byte offset from the (problem, head) base inside one descriptor: keys behind it would read as zeros
    const int64_t kv_rs = d.k_rs > d.v_rs ? d.k_rs : d.v_rs;
    const bool kv_fits = attn_rows_fit(d.seq_k, kv_rs, d.head_dim);
    auto generic = [&](int family, int D, int nw, int qb, int kvt, bool fold, bool single, int nrep) {
        const int rows = 16 * nw * qb;
        const int64_t nqb = ((int64_t)d.seq_q + rows - 1) / rows, per = (int64_t)d.heads * (d.batch / nrep);
        if (per > 0x7fffffff || nqb * per > 0x7fffffff) return p;
        const int64_t nwg = nqb * per;
        insv2v_attention_plan_t r = {};
        r.rc = 0; r.family = family;
        r.d = D; r.nw = nw; r.qb = qb; r.kvt = kvt; r.fold = fold;
        r.threads = nw * 64; r.grid = (int32_t)nwg;
        r.lds_bytes = (int32_t)attn_lds_bytes(D, kvt, single);
        r.rows_per_wg = (int64_t)rows * nrep > 0x7fffffff ? 0x7fffffff : rows * nrep;
        r.ntiles = (int32_t)(((int64_t)d.seq_k + kvt - 1) / kvt);
        r.ragged = d.seq_k % kvt != 0;
        return r;
    };
    // d = 512 (the VAE's one-head mid block): one form for every sequence length.  Plain softmax only.
    if (d.head_dim == 512) {
        if (d.causal || biased || !kv_fits) return p;
        return generic(INSV2V_ATTN_PLAN_D512, 512, 4, 1, 32, false, false, 1);
    }
    // <= 16 queries and keys (temporal attention over the frames): one wave per head, no K tile in LDS
    if ((sw.short_on || biased) && d.seq_q <= ATTN_SHORT_ROWS && d.seq_k <= ATTN_SHORT_ROWS && !d.causal && d.heads <= ATTN_SHORT_MAX_HEADS) {
        bool ok = attn_head_dim_ok(d.head_dim);
        const int64_t lds = attn_short_lds_bytes(d.heads, d.head_dim);
        ok = ok && lds <= ATTN_SHORT_LDS_MAX;                                           // beyond it: the generic form (unbiased problems only)
        ok = ok && !(biased && d.heads * 64 > ATTN_SHORT_MAXT);                          // the biased form is compiled for <= 8 heads
        if (ok) {
            if (!attn_rows_fit(d.seq_k, d.v_rs, d.head_dim)) return p;                  // only V goes through a descriptor here
            // the biased form is persistent over problems (its bias fragments are read once per wave): a few workgroups per CU.  Without a
            // CU count (cus <= 0) or with short_wgs = 0: one workgroup per problem
            int64_t grid = d.batch;
            if (biased && sw.short_wgs > 0 && cus > 0 && (int64_t)cus * sw.short_wgs < grid) grid = (int64_t)cus * sw.short_wgs;
            p.rc = 0; p.family = biased ? INSV2V_ATTN_PLAN_SHORT_BIAS : INSV2V_ATTN_PLAN_SHORT;
            p.d = d.head_dim; p.nw = d.heads; p.qb = 1; p.kvt = ATTN_SHORT_ROWS; p.fold = 0;
            p.threads = d.heads * 64; p.grid = (int32_t)grid;
            p.lds_bytes = (int32_t)lds;
            const int64_t rows = (int64_t)ATTN_SHORT_ROWS * d.heads * ((d.batch + grid - 1) / grid);
            p.rows_per_wg = rows > 0x7fffffff ? 0x7fffffff : (int32_t)rows;
            p.ntiles = 1;
            p.ragged = d.seq_k < ATTN_SHORT_ROWS;
            return p;
        }
    }
    if (biased) return p;   // only the <= 16-row kernel adds the tables: never silently drop them
    if (!attn_head_dim_ok(d.head_dim) || !kv_fits) return p;
    // the 96-token spatial self- / text cross-attention of the 8x12 level (d = 160): one workgroup of six waves per (frame, head), the
    // whole key sequence as one 96-key tile in a single LDS buffer.  Its 16-byte output stores need 16-byte aligned output rows.
    const int oa = ATTN_SINGLE_O_ALIGN / 2 - 1;
    const bool o16 = !(d.o_rs & oa) && !((uintptr_t)d.o & (ATTN_SINGLE_O_ALIGN - 1)) && !(d.o_outer & oa) && !(d.o_step & oa);
    if (sw.single && o16 && d.head_dim == 160 && !d.causal && d.seq_q > 64 && d.seq_q <= ATTN_SINGLE_KVT && d.seq_k <= ATTN_SINGLE_KVT) {
        // consecutive problems sharing one K / V (text cross-attention: the frames of a sample): one workgroup per (sample, head) keeps the tile
        if (sw.rep && d.kv_inner > 1 && d.kv_step == 0 && d.batch % d.kv_inner == 0)
            return generic(INSV2V_ATTN_PLAN_SINGLE_REP, 160, 6, 1, ATTN_SINGLE_KVT, false, true, d.kv_inner);
        return generic(INSV2V_ATTN_PLAN_SINGLE, 160, 6, 1, ATTN_SINGLE_KVT, false, true, 1);
    }
    // 16 query rows per wave and query block: short query sequences (temporal, seq = frames) use 1-wave workgroups; long ones 4 or 8
    // waves x 2 query blocks
    int nw = 4, qb = 1;
    if (d.seq_q <= 16) nw = 1;
    else if (d.seq_q <= 32) nw = 2;
    else if (d.seq_q >= 512 && d.seq_q % 256 == 0 && d.head_dim <= 96) { nw = 8; qb = 2; }
    else if (d.seq_q >= 128 && d.head_dim <= 96) qb = 2;
    const bool fold = sw.fold && (d.head_dim == 40 || d.head_dim == 80) && nw >= 4;   // (INSV2V_ATTN_FOLD=0: the unfolded form, for A/B)
    return generic(INSV2V_ATTN_PLAN_GENERIC, d.head_dim, nw, qb, attn_kvt(nw), fold, false, 1);
}
