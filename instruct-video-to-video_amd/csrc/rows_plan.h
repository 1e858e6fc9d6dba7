// The dispatch of insv2v_rowlin as a pure function: plan_rowlin(descriptor, tb2 mask, cus) -> insv2v_rowlin_plan_t.
// Host-only, no HIP call, no static, no environment read.  insv2v_rowlin validates through it, then launches what it says;
// insv2v_rowlin_plan returns it without touching a GPU.  The geometry below is the kernels' own (rows_ffn.hip static_asserts it).
#pragma once
#include <stdint.h>
#include "../../include/insv2v_hip.h"

constexpr int ROWLIN_TILE_ROWS = 128;            // rows of a workgroup's tile per token block (4 waves x 32 tokens)
constexpr int ROWLIN_SLOT_BYTES = 16 * 1024;     // one ring slot: 16 fragments of 1 KiB
constexpr int ROWLIN_MAX_FRAMES = 16;            // rows of the per-frame bias table (one one-hot k-step)
// K = 640 forms that run two token blocks per wave: bit (LN << 2 | FRAME << 1 | RES); measured per form, profiles/r03_rowlin_tb2.txt
constexpr int ROWLIN_TB2_DEFAULT = 0xff;

constexpr bool rowlin_k_ok(int K) { return K == 320 || K == 640; }
constexpr int rowlin_wgs_per_cu(int ks) { return ks <= 20 ? 2 : 1; }                 // LinCfg<KS>::WGS
constexpr int rowlin_ring_slots(int ks, bool gn) { return ks <= 20 ? 4 : gn ? 8 : 9; }   // lin_ring_slots<KS, GN>()
// dynamic LDS: the ring; the GroupNorm-on-load form adds the four waves' (scale, shift) tables of 16 KS pairs behind it
constexpr int rowlin_lds_bytes(int ks, bool gn) { return rowlin_ring_slots(ks, gn) * ROWLIN_SLOT_BYTES + (gn ? 4 * 16 * ks * 8 : 0); }

static inline insv2v_rowlin_plan_t plan_rowlin(const insv2v_rowlin_desc& d, int tb2_mask, int cus) {
    insv2v_rowlin_plan_t p = {};
    p.rc = INSV2V_EINVAL;
    if (!d.x || !d.out || !d.wstream || d.M <= 0 || d.N <= 0) return p;
    p.rc = INSV2V_EUNSUPPORTED;
    if (!rowlin_k_ok(d.K) || (d.N & 63)) return p;
    if (d.frame_bias && (d.rows_per_frame <= 0 || d.frames <= 0 || d.frames > ROWLIN_MAX_FRAMES)) return p;
    p.rc = INSV2V_EINVAL;
    if ((d.ldx & 7) || (d.ldo & 7) || ((uintptr_t)d.x & 15) || ((uintptr_t)d.out & 15) || ((uintptr_t)d.wstream & 15)) return p;
    if (d.residual && ((d.ldr & 7) || ((uintptr_t)d.residual & 15))) return p;
    p.rc = INSV2V_EUNSUPPORTED;
    // (descriptors are rebased per 128/256-row tile: only a tile's own extent has to fit the 2 GiB window, the operands may be larger)
    const int64_t lim = (int64_t)1 << 31;
    if (256 * (int64_t)d.ldx * 2 >= lim || 256 * (int64_t)d.ldo * 2 >= lim || (d.residual && 256 * (int64_t)d.ldr * 2 >= lim)) return p;
    p.ks = d.K / 16;
    p.form = (d.layernorm ? 4 : 0) | (d.frame_bias ? 2 : 0) | (d.residual ? 1 : 0);
    p.gn = d.gn_ab != nullptr;
    p.token_blocks = 1;
    int64_t ntiles = ((int64_t)d.M + ROWLIN_TILE_ROWS - 1) / ROWLIN_TILE_ROWS;
    if (p.gn) {
        if (d.gn_rows <= 0 || ((uintptr_t)d.gn_ab & 15)) return p;
        // every sample (the last one may be partial) gets its own 32-row wave blocks, four of them to a tile
        p.gn_units = (d.gn_rows + 31) / 32;
        const int64_t blocks = ((int64_t)d.M + d.gn_rows - 1) / d.gn_rows * p.gn_units;
        if ((blocks + 3) / 4 * ROWLIN_TILE_ROWS >= lim) return p;
        ntiles = (blocks + 3) / 4;
        if (p.form != 0) return p;   // fused input GroupNorm: only the plain form (proj_in of the transformer blocks) exists
    } else if (p.ks == 40 && ((tb2_mask >> p.form) & 1) && ((int64_t)d.M + 255) / 256 >= 2 * (int64_t)cus) {
        // two token blocks per wave where the register file holds them, and only where the launch keeps >= 2 rounds of 256-row tiles
        // (5 stacked clips at level 1 = 1.4 rounds: slower, profiles/r03_rowlin_tb2.txt)
        p.token_blocks = 2;
        ntiles = ((int64_t)d.M + 255) / 256;
    }
    p.tile_rows = ROWLIN_TILE_ROWS * p.token_blocks;
    p.ntiles = (int32_t)ntiles;
    p.wgs_per_cu = rowlin_wgs_per_cu(p.ks);
    p.lds_bytes = rowlin_lds_bytes(p.ks, p.gn);
    const int64_t slots = (int64_t)cus * p.wgs_per_cu;
    if (slots <= 0) { p.rc = INSV2V_EINVAL; return p; }   // (the persistent grid is sized by the CU count)
    p.grid = (int32_t)(ntiles < slots ? ntiles : slots);
    p.rounds = (int32_t)((ntiles + p.grid - 1) / p.grid);
    p.rc = 0;
    return p;
}
