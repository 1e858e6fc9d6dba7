// The dispatch of insv2v_groupnorm as a pure function: plan_groupnorm(descriptor, switches) -> insv2v_groupnorm_plan_t.
// Host-only, no HIP call, no static, no environment read.  insv2v_groupnorm validates through it, then launches what it says;
// insv2v_groupnorm_plan returns it without touching a GPU.  The limits below are the kernels' own (norm.hip static_asserts them).
#pragma once
#include <stdint.h>
#include "../../include/insv2v_hip.h"

constexpr int GN_SMALL_MAXCH = 16;             // gn_small_kernel: chunks per thread (GNS_MAXCH), 256 threads
constexpr int GN_SMALL_LDS = (8 + 2 * 256) * 4;   // its static LDS: two reductions of 4 waves, the group's gamma and beta
constexpr int GN_FRAME_MAXCH = 15;             // gn_frame_kernel: 16-byte chunks per thread (GNF_MAXCH)
constexpr int GN_FRAME_LDS_MAX = 96 * 1024;    // the dynamic LDS it is allowed
constexpr int GN_PARTIAL_LDS_MAX = 64 * 1024;  // gn_partial_kernel: P x C Moments of 12 bytes
constexpr int GN_MOMENTS_BYTES = 12;

// The A/B switches of the GroupNorm dispatch, read once (insv2v_groupnorm_switches, norm.hip).  Defaults = the product.
struct groupnorm_switches {
    int frame = 1;   // INSV2V_GN_FRAME: the whole-sample kernel by dispatch
    int split = 0;   // INSV2V_GN_FRAME_SPLIT: > 0 overrides its channel split (1 = one workgroup per sample)
};

static inline bool gn_pow2(int v) { return v > 0 && !(v & (v - 1)); }

static inline insv2v_groupnorm_plan_t plan_groupnorm(const insv2v_groupnorm_desc& d, const groupnorm_switches& sw) {
    insv2v_groupnorm_plan_t p = {};
    p.family = INSV2V_GN_PLAN_NONE;
    p.rc = INSV2V_EINVAL;
    if (!d.x || !d.gamma || !d.beta || !d.partials) return p;
    if (d.stats_only ? !d.ab : !d.y) return p;
    if (d.C <= 0 || d.G <= 0 || (d.C % d.G) || (d.C & 7) || d.C > 8192) return p;
    if ((d.ldx & 7) || (d.ldy & 7) || d.nsamples <= 0 || d.rows_per_sample <= 0) return p;
    if (d.x2 && ((d.C1 & 7) || d.C1 <= 0 || d.C1 >= d.C || (d.ldx2 & 7))) return p;
    if (d.nchunks <= 0) return p;
    const int cpg = d.C / d.G;
    const int64_t nchunk = (int64_t)d.rows_per_sample * (d.C / 8);
    // whole samples of <= 245 KB (the per-frame GroupNorm of the 8x12 / 4x6 levels), many of them: one workgroup per sample and channel part
    if (sw.frame && !d.stats_only && !d.ab && !d.x2 && (cpg % 8) == 0 && d.nsamples >= 128 && nchunk >= 2048 && nchunk <= 1024 * GN_FRAME_MAXCH &&
        (d.G == 32 || d.G == 16) && d.C <= 2560) {
        // channel split CS (see the kernel): as many parts as keep whole groups and >= 1024 chunks per workgroup ...
        int CS = sw.split > 0 ? sw.split : (nchunk > 512 * GN_FRAME_MAXCH ? 4 : nchunk > 256 * GN_FRAME_MAXCH ? 2 : 1);
        int NT = 0;
        bool ok = false;
        for (;;) {
            while (CS > 1 && (d.G % CS || nchunk / CS < 1024)) CS >>= 1;
            const int64_t nc = nchunk / CS;
            NT = nc <= 256 * GN_FRAME_MAXCH ? 256 : nc <= 512 * GN_FRAME_MAXCH ? 512 : 1024;
            // ... and the kernel's reduction contract: the NT / (G / CS) threads of a group are a power of two inside one wave.  Every
            // split the dispatch chooses by itself meets it; an override that does not (G = 16 in 8 parts: 128 threads per group) is halved
            const int Gw = d.G / CS;
            ok = NT % Gw == 0 && NT / Gw <= 64 && gn_pow2(NT / Gw) && nc <= (int64_t)NT * GN_FRAME_MAXCH;
            if (ok || CS == 1) break;
            CS >>= 1;
        }
        const int64_t lds = ((int64_t)d.rows_per_sample * (d.C / CS / 8) + 2 * (d.G / CS) + 2 * (d.C / CS)) * 4;
        if (ok && lds <= GN_FRAME_LDS_MAX) {
            p.rc = 0; p.family = INSV2V_GN_PLAN_FRAME;
            p.nt = NT; p.cs = CS; p.threads = NT;
            p.nchunks = 1; p.rows_per_chunk = d.rows_per_sample;
            p.apply_grid_x = d.nsamples;
            p.lds_bytes = (int32_t)lds;
            return p;
        }
    }
    {   // small slabs: one launch, one read + one write (cpg*2 B >= 32 B keeps the strided row pieces sector-sized)
        const int vw = (cpg % 8 == 0) ? 8 : ((cpg % 4 == 0) ? 4 : 0);
        const bool src_ok = !d.x2 || (d.C1 % (vw ? vw : 1) == 0);
        if (!d.stats_only && !d.ab && vw && cpg >= 16 && cpg <= 256 && src_ok && (int64_t)d.rows_per_sample * (cpg / vw) <= 256 * GN_SMALL_MAXCH) {
            p.rc = 0; p.family = INSV2V_GN_PLAN_SMALL;
            p.vw = vw; p.threads = 256;
            p.nchunks = 1; p.rows_per_chunk = d.rows_per_sample;
            p.apply_grid_x = d.G;
            p.lds_bytes = GN_SMALL_LDS;
            return p;
        }
    }
    p.rc = INSV2V_EUNSUPPORTED;
    const int CC = d.C / 8;
    if (CC > 1024) return p;
    int P = 256 / CC;
    if (P < 1) P = 1;
    if (P > 16) P = 16;
    const int64_t lds = (int64_t)P * d.C * GN_MOMENTS_BYTES;
    if (lds > GN_PARTIAL_LDS_MAX) return p;
    p.rc = 0; p.family = INSV2V_GN_PLAN_THREE_PASS;
    p.p = P; p.threads = CC * P;
    p.nchunks = d.nchunks < d.rows_per_sample ? d.nchunks : d.rows_per_sample;
    p.rows_per_chunk = (d.rows_per_sample + p.nchunks - 1) / p.nchunks;   // a trailing chunk may be empty when rows do not divide: it contributes n = 0
    p.lds_bytes = (int32_t)lds;
    if (!d.stats_only) {
        const long want = ((long)d.rows_per_sample + P * 4 - 1) / (P * 4);
        long cap = 4096 / d.nsamples;
        if (cap < 1) cap = 1;
        p.apply_grid_x = (int32_t)(want < cap ? want : cap);
    }
    return p;
}
