// The dispatch of insv2v_gemm as a pure function: plan_gemm(descriptor, CU count, operand window, switches) -> insv2v_gemm_plan_t.
// Host-only, no HIP call, no static, no environment read.  insv2v_gemm validates, plans and executes the plan; insv2v_gemm_plan,
// insv2v_gemm_stats_parts and insv2v_conv3x3_fuses_groupnorm read the same plan; the three engines' entries (gemm_q8 / gemm_r8 /
// gemm_w4.hip) refuse by the predicates below, which the planner asks first - it never plans an engine that would refuse.
// DESIGN.md section 3 has the rule order as a table.
#pragma once
#include <stdint.h>
#include <algorithm>
#include "../../include/insv2v_hip.h"

constexpr int GEMM_BK = 64;   // halfs per K slice of the tile / patch-tiled / 8-wave ping-pong kernels (BK, gemm_dma.h)
constexpr int W4_BK = 32;     // of gemm_w4 (BK4)

// The A/B switches of the GEMM path, read once (insv2v_gemm_switches, gemm.hip).  Defaults = the product.
struct gemm_switches {
    int r8 = 1;               // INSV2V_GEMM_R8: the 8-wave ping-pong kernels (gemm_q8 / gemm_r8) by dispatch
    int r8_stats = 1;         // INSV2V_R8_STATS: gemm_r8 emits the output rows' statistics
    int q8_min_n = 256;       // INSV2V_Q8_MIN_N: the narrowest output gemm_q8 takes by dispatch
    int persistent = 1;       // INSV2V_GEMM_PERSISTENT: the measured shape rules of persistent_choice and of the big convolutions
    int r8_geglu = 1;         // INSV2V_R8_GEGLU: the GEGLU FF1 on gemm_r8
    int r8_cim = 1;           // INSV2V_R8_CIM: stride-1 / pad-1 convolutions on gemm_r8 walk K channel-block-major
    int halo_legacy_map = 0;  // INSV2V_HALO_LEGACY_MAP: the patch-tiled kernel's earlier tile map
    int r8_dephase = 0;       // INSV2V_R8_DEPHASE: permille of a tile time over which the workgroups with one tile to spare start late
    int w4_wgs = 2, w4_delay = -1;   // INSV2V_W4_WGS, INSV2V_W4_DELAY: debugging (workgroups per CU, tile delay)
};
const gemm_switches& insv2v_gemm_switches();

static inline void gemm_defaults(insv2v_gemm_desc& d) { if (d.batch <= 0) d.batch = 1; if (d.alpha == 0.f) d.alpha = 1.f; }
static inline bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }
static inline bool beyond_2g(int64_t bytes) { return bytes >= ((int64_t)1 << 31); }

// ---- eligibility of the three persistent engines: 0, or the code the engine's entry returns ------------------------------------------
// The engines park ONE row-bias vector per tile: every bm-row tile must lie inside one bias group.
static inline bool row_bias_fits_tiles(const insv2v_gemm_desc& d, int bm) { return !d.row_bias || !((d.ld_rb & 3) || (d.rows_per_group % bm && d.M > d.rows_per_group)); }
// what all three ask of the operands (bk: their K slice)
static inline bool engine_operands_ok(const insv2v_gemm_desc& d, int bk) {
    if (d.batch > 1 || d.c_fp32 || d.split_k > 1) return false;
    if ((d.K % bk) || (d.N & 7) || (d.ldc & 7) || misaligned16(d.c)) return false;
    if (d.residual && ((d.ldr & 7) || misaligned16(d.residual))) return false;
    if (d.k_split && (d.k_split % bk)) return false;
    if (d.act != INSV2V_ACT_NONE && d.act != INSV2V_ACT_GEGLU) return false;   // SiLU / quick-GELU GEMMs are tiny (time embedding, CLIP)
    if (d.row_stats && (d.M & 1)) return false;                                  // (mean, rstd) pairs are fetched two rows per lane
    if (beyond_2g((int64_t)d.M * d.ldc * 2) || (d.residual && beyond_2g((int64_t)d.M * d.ldr * 2))) return false;
    if (d.act == INSV2V_ACT_GEGLU && ((d.N % 64) || d.mode == INSV2V_MODE_CONV3X3 || d.residual)) return false;
    return !(d.mode == INSV2V_MODE_CONV3X3 && (d.Cin % bk));
}
// gemm_q8: 256x256.  variant: 0 = product (LDS-DMA requests inside the MFMA segments); 1 = requests in the load segments (round-4 A/B:
// 5-18 % slower); 2 = no epilogue (timing); 3 = the two wave groups' epilogues one after the other (A/B); 4 / 5 = stamps of schedule 1 / 0
static inline int q8_refusal(const insv2v_gemm_desc& d, int variant) {
    const bool conv = d.mode == INSV2V_MODE_CONV3X3, gg = d.act == INSV2V_ACT_GEGLU, res = d.residual != nullptr;
    if (!engine_operands_ok(d, GEMM_BK) || !row_bias_fits_tiles(d, 256)) return INSV2V_EUNSUPPORTED;
    if (variant < 0 || variant > 5) return INSV2V_EINVAL;
    return (variant == 3 ? conv : variant >= 2 && (conv || gg || res)) ? INSV2V_EUNSUPPORTED : 0;
}
// gemm_r8: 256x320.  variant: 0 = product; 2 / 5 = no epilogue (timing); 4 = cycle stamps
static inline int r8_refusal(const insv2v_gemm_desc& d, int variant) {
    const bool conv = d.mode == INSV2V_MODE_CONV3X3, gg = d.act == INSV2V_ACT_GEGLU;
    if (!engine_operands_ok(d, GEMM_BK) || !row_bias_fits_tiles(d, 256)) return INSV2V_EUNSUPPORTED;
    // GEGLU (W rows in [32 value | 32 gate] blocks) and partial row statistics of the output: LINEAR, whole 320-row / column tiles, one A
    // source, the product variant, and not both
    if ((gg || d.stats_out) && (conv || (d.N % 320) || d.k_split > 0 || variant != 0 || (gg && d.stats_out))) return INSV2V_EUNSUPPORTED;
    if ((d.bias && misaligned16(d.bias)) || (d.col_sum && misaligned16(d.col_sum)) || (d.row_bias && misaligned16(d.row_bias))) return INSV2V_EUNSUPPORTED;
    if (conv && d.M >= (1 << 24)) return INSV2V_EUNSUPPORTED;   // (row -> pixel by fp32 division: exact below 2^24 rows)
    return (variant == 0 || variant == 2 || variant == 4 || variant == 5) ? 0 : INSV2V_EINVAL;
}
// stride-1 / pad-1 convolutions (every ResnetBlock3D convolution) on gemm_r8 walk K channel-block-major (template flag CIM);
// INSV2V_R8_CIM=0 keeps the tap-major order for A/B runs
static inline bool r8_uses_cim(const insv2v_gemm_desc& d, int variant, const gemm_switches& sw) {
    return d.mode == INSV2V_MODE_CONV3X3 && sw.r8_cim && !d.stats_out && (variant == 0 || variant == 4) && d.stride == 1 && !d.upsample && d.pad_t == 1 &&
           d.pad_l == 1 && d.IH == d.OH && d.IW == d.OW;
}
// gemm_w4.  variant % 10: 0 = 4 waves 128x256, 1 = 4 waves 256x128, 2 = 8 waves 128x256, 3 = 8 waves 256x128; +10 = timing ablation without epilogue
static inline int w4_refusal(const insv2v_gemm_desc& d, int variant) {
    const int v = variant % 10;
    if (!engine_operands_ok(d, W4_BK) || d.K < 2 * W4_BK) return INSV2V_EUNSUPPORTED;
    if (v >= 2 && d.act == INSV2V_ACT_GEGLU) return INSV2V_EUNSUPPORTED;   // the 8-wave tiles exist for the memory-bound N = C GEMMs
    if (!row_bias_fits_tiles(d, (v == 1 || v == 3) ? 256 : 128)) return INSV2V_EUNSUPPORTED;
    if (v < 0 || v > 3) return INSV2V_EINVAL;
    return (variant / 10 == 1 && d.mode == INSV2V_MODE_CONV3X3) ? INSV2V_EUNSUPPORTED : 0;   // (the ablation is LINEAR only)
}

// ---- the rules --------------------------------------------------------------------------------------------------------------------------
// tile shapes of the tile kernel: 1 = 128x128, 2 = 64x128, 3 = 128x64, 4 = 64x64 (4 waves); 5 = 128x128, 6 = 256x128, 7 = 128x64 (8 waves);
// 8 = 128x128, 9 = 128x64 (8 waves as 2 K groups of 4)
static inline int tile_bm(int shape) { return shape == 6 ? 256 : (shape == 2 || shape == 4) ? 64 : 128; }
static inline int tile_bn(int shape) { return (shape == 3 || shape == 4 || shape == 7 || shape == 9) ? 64 : 128; }
constexpr size_t tile_lds_bytes(int bm, int bn, int stages) {
    const size_t ring = (size_t)stages * (bm + bn) * GEMM_BK * 2, stage = (size_t)bm * (bn + 4) * sizeof(float);
    return (ring > stage ? ring : stage) + (size_t)(2 * bn + 2 * bm) * sizeof(float);
}
constexpr size_t TILE_LDS_MAX = 160 * 1024;
static inline int pick_tile(const insv2v_gemm_desc& d) {
    // Measured on MI355X (tools/bench_gemm.py, profiles/): the kernel is bound by memory latency x the LDS
    // capacity available for slices in flight, so wave-level parallelism decides: the 8-wave 128x128 tile
    // (2 workgroups = 16 waves per CU) wins whenever it yields >= ~200 workgroups; tiny problems
    // (M = 1152 at the lowest UNet level) use 64x64 tiles (4-5 workgroups/CU).
    // GEGLU needs each wave to own an [h|g] pair of 32-row weight blocks (NI = 2): tiles 5 / 2.
    const long batch = d.batch > 0 ? d.batch : 1;
    auto blocks = [&](int bm, int bn) { return (long)((d.M + bm - 1) / bm) * ((d.N + bn - 1) / bn) * batch; };
    const long b11 = blocks(128, 128);
    if (d.act == INSV2V_ACT_GEGLU) return b11 >= 200 ? 5 : 2;
    if (d.mode == INSV2V_MODE_CONV3X3) return (b11 >= 200 && d.N >= 128) ? 5 : 4;
    // Round 2 re-check (profiles/r02_ring_depth_tile_sweep.txt): in ISOLATION the 64x64 tile wins on the single-branch N = C GEMMs
    // (1536 x 1280 x 1280 + residual 15.0 vs 19.3 us, 24 576 x 320 x 320 17.8 vs 20.1 us), but a rule that picked it there made the
    // 3-stream UNet step SLOWER (-2.7 % vs -4.3 % against the same baseline): three branches' kernels overlap, and many small
    // workgroups crowd the other branches' tiles out.  Deeper LDS rings (tile codes 3x / 4x) lose wherever they cost a workgroup per CU.
    return blocks(128, 64) >= 200 ? 5 : 4;
}

// The "rounds of tiles" cost of the two 8-wave ping-pong kernels (persistent grids of one workgroup per CU): rounds x tile width, and
// gemm_q8's 16x16x32 engine 3 % behind gemm_r8's per column (tools/gemm_check --set unet30: profiles/r04_gemm_r8_unet30.txt).
struct pingpong_cost { double q8, r8; };
static inline pingpong_cost pingpong_costs(const insv2v_gemm_desc& d, int cus) {
    const long tm = (d.M + 255) / 256;
    auto rounds = [&](int bn) { return (double)((tm * ((d.N + bn - 1) / bn) + cus - 1) / cus) * bn; };
    return {rounds(256) * 1.03, rounds(320)};
}
// Round 4: which of the two 8-wave ping-pong kernels (gemm_q8: 256x256, gemm_r8: 256x320) - if any - runs a linear GEMM without
// activation or a convolution.  Every UNet width is a multiple of 320, so gemm_r8 has no partial column tiles where gemm_q8 has
// (N = 320 / 640 / 960 / 1920); what decides is how the tile count quantises over the CUs (persistent grids: rounds of tiles), against
// the finer-grained round-1 kernels (128x128 tiles / patch-tiled conv, two workgroups per CU) at ~0.8 of the new engine's rate
// (tools/gemm_check --set unet30: profiles/r04_gemm_r8_unet30.txt).  stats: the problem emits its output rows' statistics.
// Returns 0 = neither, 1 = gemm_q8, 2 = gemm_r8.
static inline int pingpong_choice(const insv2v_gemm_desc& d, bool stats, int cus, const gemm_switches& sw) {
    if (!sw.r8 || d.act != INSV2V_ACT_NONE || d.batch > 1 || d.c_fp32 || d.M < 8192 || d.N < 256) return 0;
    // statistics of the output rows: only gemm_r8's LINEAR form emits them (two 160-column partial sums per tile row)
    if (stats && (!sw.r8_stats || d.mode != INSV2V_MODE_LINEAR || d.k_split || (d.N % 320))) return 0;
    if (d.mode == INSV2V_MODE_LINEAR && d.K < 256) return 0;
    if (!row_bias_fits_tiles(d, 256) || cus <= 0) return 0;
    const double old_cost = (double)((d.M + 255) / 256) * d.N / cus / 0.80;
    const pingpong_cost c = pingpong_costs(d, cus);
    // (only the UNet's widths: the VAE's 128 / 256 / 512-channel convolutions stay where round 3 measured them)
    if (d.N % 320 == 0 && (c.r8 <= c.q8 || stats) && c.r8 < old_cost) return 2;
    // (INSV2V_Q8_MIN_N: the narrowest output gemm_q8 takes by dispatch; round 6: 256, i.e. the VAE's 256 / 512-channel
    //  convolutions on the 16x16x32 engine: profiles/r06_vae_q8_ab.txt)
    if (d.N % 256 == 0 && d.N >= sw.q8_min_n && (d.N % 320 != 0 || c.q8 < c.r8) && c.q8 < old_cost && d.K >= 1152 && !stats) return 1;
    return 0;
}
// Persistent big-tile kernels (gemm_q8.hip: 256x256, one 8-wave workgroup per CU; gemm_w4.hip: 128x256, two 4-wave workgroups per CU)
// for the linear shapes where they measured faster than the 128x128 tile on MI355X (tools/gemm_check, profiles/r02_gemm_check_*.txt;
// both the 3-branch batched and the single-branch token counts): the GEGLU FF1 and the fused q/k/v projections, i.e. wide-N GEMMs
// without a residual.  GEMMs with a residual (N = C) and every convolution stay on the 2-workgroup 128x128 / halo kernels, whose four
// waves per SIMD overlap the epilogue with the next tile.  Returns 0 = no, 1 = gemm_q8 (round 4: it took over the 256x256 choices of
// round 3's gemm_p8, 8-25 % faster on every UNet shape, profiles/r04_gemm_q8_vs_p8.txt), 2 = gemm_w4.
static inline int persistent_choice(const insv2v_gemm_desc& d, const gemm_switches& sw) {
    if (!sw.persistent || d.mode != INSV2V_MODE_LINEAR || d.batch > 1 || d.c_fp32 || d.k_split) return 0;
    if (!row_bias_fits_tiles(d, 256)) return 0;
    // Round 3 (stacked clips, M = 23 040 ... 92 160 at levels 1-2): with K >= 1280 the 256x256 kernel's epilogue is amortised and it
    // wins with or without a residual - FF2 23 040 x 1 280 x 5 120 358 vs 424 us, q/k/v 23 040 x 3 840 x 1 280 259 vs 325 us, FF2
    // 92 160 x 640 x 2 560 462 vs 482 us; at the single-clip sizes (M*N below ~2e7) the 128x128 tile stays ahead
    // (tools/bench_tiles_r03.py, profiles/r03_tile_sweep_stacked.txt)
    // (N = 640 - FF2 of level 1 - is 2.5 column tiles of the 256x256 kernel; running the last 128 columns on the 128x128 tile as a
    //  second launch was built and measured: no gain end to end, profiles/r03_gemm_split_columns_experiment.txt)
    if (d.act == INSV2V_ACT_NONE && d.K >= 1280 && d.N >= 640 && (int64_t)d.M * d.N >= (int64_t)20 << 20) return 1;
    if (d.residual) return 0;
    if (d.act == INSV2V_ACT_GEGLU) return d.K <= 320 ? (d.M >= 8192 ? 2 : 0) : (d.M >= 1024 ? 1 : 0);
    if (d.act != INSV2V_ACT_NONE || d.N < 960 || d.K > 640 || d.M < 4096) return 0;
    return (d.M < 12288 && d.K == 640) ? 1 : 2;
}
// Automatic split-K: only for problems that cannot fill the chip (fewer than ~1 workgroup per CU with
// 128x128 tiles) and whose K is long enough that every split still runs >= 16 slices.
static inline int split_choice(const insv2v_gemm_desc& d) {
    if (d.split_k == 1 || !d.workspace || d.batch > 1 || d.act == INSV2V_ACT_GEGLU || (d.N & 7) || d.row_stats || d.rb_mod > 0) return 1;
    const long b11 = (long)((d.M + 127) / 128) * ((d.N + 127) / 128);
    const int nk = (d.K + GEMM_BK - 1) / GEMM_BK;
    int s = d.split_k;
    if (s == 0) {
        if (b11 >= 200 || nk < 64) return 1;
        s = std::min({(int)(512 / b11), nk / 16, 8});
    }
    if (s < 2) return 1;
    if ((int64_t)s * d.M * d.N * 4 > d.workspace_bytes) return 1;
    return s;
}
// Split-K main pass: raw fp32 partial slabs [nsplit, M, N] in the workspace, no epilogue (splitk_reduce applies it)
static inline void splitk_main_pass(insv2v_gemm_desc& d, int nsplit) {
    d.c = d.workspace; d.ldc = d.N; d.c_fp32 = 1; d.c_bs = 0;
    d.bias = nullptr; d.row_bias = nullptr; d.residual = nullptr; d.act = INSV2V_ACT_NONE; d.alpha = 1.f;
    d.row_stats = nullptr; d.col_sum = nullptr; d.split_k = nsplit;
}
// patch geometry of the patch-tiled (halo) kernel for this problem: log2(TW), or -1 when it does not apply
static inline int halo_tw_shift(const insv2v_gemm_desc& d) {
    if (d.mode != INSV2V_MODE_CONV3X3 || d.stride != 1 || d.pad_t != 1 || d.pad_l != 1 || (d.Cin % GEMM_BK) || d.batch > 1) return -1;
    if (d.k_split > 0 && (d.k_split % GEMM_BK)) return -1;
    if (d.row_stats || d.rb_mod > 0 || d.act == INSV2V_ACT_GEGLU) return -1;
    const int up = d.upsample ? 2 : 1;
    if (d.OH != d.IH * up || d.OW != d.IW * up) return -1;
    if (d.OH % 8 == 0 && d.OW % 16 == 0) return 4;   // 8 x 16 patch
    if (d.OH % 16 == 0 && d.OW % 8 == 0) return 3;   // 16 x 8 patch
    return -1;
}
// the patch-tiled kernel by dispatch: once its 128-pixel patches x 128-column tiles give the chip >= ~200 workgroups
static inline bool halo_fills_chip(const insv2v_gemm_desc& d) { return ((long)d.M / 128) * ((d.N + 127) / 128) >= 200; }

// Column-tile width of the kernel that runs this problem when it emits its rows' statistics (0 = cannot emit): such a problem always
// takes gemm_r8's LINEAR form or the tile kernel's vectorised fp16 epilogue, no split-K, no other persistent kernel.
static inline int stats_width_of(const insv2v_gemm_desc& d, int cus, const gemm_switches& sw) {
    if (d.mode != INSV2V_MODE_LINEAR || d.c_fp32 || d.act == INSV2V_ACT_GEGLU || d.batch > 1 || (d.N & 7) || (d.ldc & 7) || misaligned16(d.c) ||
        (d.residual && ((d.ldr & 7) || misaligned16(d.residual) || beyond_2g((int64_t)d.M * d.ldr * 2))))
        return 0;
    if (d.tile >= 240 && d.tile <= 249) return (d.N % 320 || d.k_split) ? 0 : 160;   // gemm_r8 forced
    if (d.tile >= 100) return 0;
    if (d.tile == 0 && pingpong_choice(d, true, cus, sw) == 2) return 160;
    const int shape = d.tile % 10 ? d.tile % 10 : pick_tile(d);
    return shape >= 1 && shape <= 9 ? tile_bn(shape) : 0;
}

// Does an operand of this problem reach beyond one window (insv2v_gemm then runs it as row / image ranges, without output statistics)?
static inline bool beyond_window(const insv2v_gemm_desc& d, int64_t window) {
    const int64_t a_rows = d.mode == INSV2V_MODE_CONV3X3 ? (int64_t)d.NB * d.IH * d.IW : (int64_t)d.M, esz = d.c_fp32 ? 4 : 2;
    const int64_t big_in = std::max(a_rows * d.lda * 2, d.k_split ? a_rows * d.lda2 * 2 : (int64_t)0);
    const int64_t big_out = std::max((int64_t)d.M * d.ldc * esz, d.residual ? (int64_t)d.M * d.ldr * 2 : (int64_t)0);
    return big_in >= window || big_out >= window;
}
// Rows (LINEAR) / images (CONV3X3) per part of a problem beyond the window: every part inside the window and aligned to the row-bias /
// GroupNorm / weight groups, parts as even as possible (every distinct part size is its own dispatch decision, equal sizes share it).  0 = no such split.
static inline int64_t units_per_part(const insv2v_gemm_desc& d, int64_t window) {
    const bool conv = d.mode == INSV2V_MODE_CONV3X3;
    auto lcm = [](int64_t a, int64_t b) { int64_t x = a, y = b; while (y) { const int64_t t = x % y; x = y; y = t; } return a / x * b; };
    const int64_t opix = conv ? (int64_t)d.OH * d.OW : 1, ipix = conv ? (int64_t)d.IH * d.IW : 1;   // output / input rows per unit
    int64_t unit = conv ? 1 : 2;                                                                 // a multiple of this
    if (d.row_bias) {
        const int64_t grp = (int64_t)d.rows_per_group * (d.rb_mod > 0 ? d.rb_mod : 1);         // rows after which the bias pattern repeats / moves on
        if (conv && grp % opix) return 0;
        unit = lcm(unit, conv ? grp / opix : grp);
    }
    if (conv && d.gn_ab) unit = lcm(unit, d.gn_images_per_sample);
    if (!conv && unit < 256) unit = lcm(unit, 256);                                             // whole tiles where nothing else decides
    if (d.w_group_rows > 0) unit = lcm(unit, d.w_group_rows);                                   // grouped weights: whole groups per part
    const int64_t total = conv ? d.NB : d.M, esz = d.c_fp32 ? 4 : 2;
    const int64_t in_row = std::max((int64_t)d.lda * 2, d.k_split ? (int64_t)d.lda2 * 2 : (int64_t)0) * ipix;
    const int64_t out_row = std::max((int64_t)d.ldc * esz, d.residual ? (int64_t)d.ldr * 2 : (int64_t)0) * opix;
    const int64_t per = (window - 1) / std::max(in_row, out_row) / unit * unit;
    if (per <= 0) return 0;
    const int64_t nparts = (total + per - 1) / per;
    return ((total + nparts - 1) / nparts + unit - 1) / unit * unit;
}

// part [u0, u0 + nu) of such a problem (units: rows / images), the same problem in every other respect
static inline insv2v_gemm_desc window_part(const insv2v_gemm_desc& f, int64_t u0, int64_t nu) {
    const bool conv = f.mode == INSV2V_MODE_CONV3X3;
    const int64_t opix = conv ? (int64_t)f.OH * f.OW : 1, ipix = conv ? (int64_t)f.IH * f.IW : 1, esz = f.c_fp32 ? 4 : 2;
    const int64_t r_in = u0 * ipix, r_out = u0 * opix;
    insv2v_gemm_desc d = f;
    d.a = (const char*)f.a + r_in * f.lda * 2;
    if (f.k_split) d.a2 = (const char*)f.a2 + r_in * f.lda2 * 2;
    d.c = (char*)f.c + r_out * f.ldc * esz;
    if (f.residual) d.residual = (const char*)f.residual + r_out * f.ldr * 2;
    if (f.row_stats) d.row_stats = f.row_stats + r_out * 2;
    if (f.w_group_rows > 0) d.w = (const char*)f.w + (r_out / f.w_group_rows) * f.w_group_stride * 2;
    if (f.row_bias && f.rb_mod <= 0) d.row_bias = f.row_bias + (r_out / f.rows_per_group) * f.ld_rb;
    if (conv && f.gn_ab) d.gn_ab = f.gn_ab + (u0 / f.gn_images_per_sample) * (int64_t)f.Cin * 2;
    d.M = (int32_t)(nu * opix); if (conv) d.NB = (int32_t)nu;
    return d;
}
// the problem once its partial row statistics are finalised into stats_scratch (ln_finalize_kernel)
static inline void stats_finished(insv2v_gemm_desc& d) { d.row_stats = d.stats_scratch; d.stats_parts = 0; }

// what insv2v_gemm refuses before any rule is asked (0 = a valid problem)
static inline int validate_gemm(const insv2v_gemm_desc& d, int stats_width) {
    if (!d.a || !d.w || !d.c || d.M <= 0 || d.N <= 0 || d.K <= 0) return INSV2V_EINVAL;
    if ((d.K & 7) || (d.lda & 7) || (d.ldw & 7)) return INSV2V_EINVAL;
    if (misaligned16(d.a) || misaligned16(d.w)) return INSV2V_EINVAL;
    if (d.k_split && (!d.a2 || (d.k_split % GEMM_BK) || (d.lda2 & 7) || misaligned16(d.a2))) return INSV2V_EINVAL;
    if (d.row_bias && d.rows_per_group <= 0) return INSV2V_EINVAL;
    if (d.row_stats && (!d.col_sum || d.batch > 1)) return INSV2V_EINVAL;
    if (d.stats_parts < 0 || (d.stats_parts > 0 && (!d.row_stats || !d.stats_scratch))) return INSV2V_EINVAL;
    if (d.stats_out && stats_width == 0) return INSV2V_EUNSUPPORTED;
    if (d.act == INSV2V_ACT_GEGLU && (d.N % 64)) return INSV2V_EINVAL;
    // (ReLU / sigmoid / tanh - the optical-flow network's - live in the tile kernel's epilogue and the split-K reduction, for both modes;
    //  the patch-tiled and persistent kernels never see those codes: the rules below keep such a call away from them)
    if (d.act < 0 || d.act > INSV2V_ACT_TANH) return INSV2V_EINVAL;   // unknown activation code
    if (d.w_group_rows < 0 || (d.w_group_rows > 0 && (d.w_group_rows % 256 || d.w_group_stride <= 0))) return INSV2V_EINVAL;
    // grouped weights: the 256-row ping-pong kernels only, nothing riding in the epilogue
    if (d.w_group_rows > 0 && (d.mode != INSV2V_MODE_LINEAR || d.batch > 1 || d.c_fp32 || d.act != INSV2V_ACT_NONE || d.residual || d.row_bias || d.row_stats ||
                               d.stats_out || d.k_split || d.split_k > 1 || d.K < 256 || (d.N % 256 && d.N % 320)))
        return INSV2V_EUNSUPPORTED;
    if (d.gn_ab && (d.mode != INSV2V_MODE_CONV3X3 || d.gn_images_per_sample <= 0 || d.upsample)) return INSV2V_EINVAL;
    if (d.mode == INSV2V_MODE_CONV3X3) {
        if (d.Cin <= 0 || (d.Cin % GEMM_BK) || d.K != 9 * d.Cin) return INSV2V_EINVAL;
        if ((long)d.NB * d.OH * d.OW != d.M || d.stride < 1) return INSV2V_EINVAL;
        // nearest-x2 upsample to an explicit output size (Upsample3D's output_size, resnet.py:41-61): the x2 image or that image without its last
        // row / column; the gather kernels zero-pad at the REQUESTED extent, and index >> 1 of any tap inside it is inside the input
        if (d.upsample && (d.stride != 1 || d.pad_t != 1 || d.pad_l != 1 || (d.OH != 2 * d.IH && d.OH != 2 * d.IH - 1) || (d.OW != 2 * d.IW && d.OW != 2 * d.IW - 1)))
            return INSV2V_EINVAL;
    } else if (d.mode != INSV2V_MODE_LINEAR) {
        return INSV2V_EUNSUPPORTED;
    }
    return beyond_2g((int64_t)d.N * d.ldw * 2) ? INSV2V_EUNSUPPORTED : 0;
}

static inline int engine_tile_code(int family) { return family == INSV2V_PLAN_R8 ? 240 : family == INSV2V_PLAN_Q8 ? 230 : 210; }   // + variant
// ---- the planner ------------------------------------------------------------------------------------------------------------------------
static inline insv2v_gemm_plan_t plan_gemm(insv2v_gemm_desc d, int cus, int64_t window, const gemm_switches& sw, bool queries_only = false) {
    insv2v_gemm_plan_t p = {};
    p.split_k = p.parts = 1;
    gemm_defaults(d);
    const bool conv = d.mode == INSV2V_MODE_CONV3X3, split = beyond_window(d, window);
    const int stats_w = stats_width_of(d, cus, sw);
    p.stats_width = split ? 0 : stats_w;   // a split problem emits no statistics: say so before the caller allocates for them
    p.gn_fuse = d.M > 0 && d.N > 0 && conv && !d.upsample && d.split_k <= 1 && (d.tile == 0 || d.tile == 100) && halo_tw_shift(d) >= 0 &&
                (d.tile == 100 || (split_choice(d) <= 1 && halo_fills_chip(d)));
    if (queries_only) return p;   // (stats_width and gn_fuse are all that insv2v_gemm_stats_parts / insv2v_conv3x3_fuses_groupnorm read)
    auto refuse = [&](int rc) { p.rc = rc; p.family = INSV2V_PLAN_NONE; return p; };
    constexpr int Q8 = INSV2V_PLAN_Q8, R8 = INSV2V_PLAN_R8, W4 = INSV2V_PLAN_W4;
    auto engine = [&](int family, int variant = 0, bool finalize = true) {   // plans an engine unless its predicate refuses: returns the refusal
        const int rc = family == R8 ? r8_refusal(d, variant) : family == Q8 ? q8_refusal(d, variant) : w4_refusal(d, variant);
        if (rc) return rc;
        p.family = family; p.variant = variant; p.forced_tile = engine_tile_code(family) + variant;
        p.ln_finalize = finalize && d.stats_parts > 0;   // these kernels park finished (mean, rstd) pairs
        p.cim = family == R8 && r8_uses_cim(d, variant, sw);
        return 0;
    };
    auto halo = [&](int cfg, int tws) { p.family = INSV2V_PLAN_HALO; p.variant = cfg; p.forced_tile = 100 + cfg; p.tw_shift = tws | (sw.halo_legacy_map ? 256 : 0); return p; };

    if (const int rc = validate_gemm(d, stats_w)) return refuse(rc);
    // LDS-DMA addressing uses 32-bit byte offsets against a 2 GiB descriptor window per operand.  A problem whose activations, output or
    // residual reach beyond one window runs as several launches over row ranges (LINEAR) / image ranges (CONV3X3: images are independent),
    // so that every kernel family keeps its 32-bit offsets; each part is planned on its own.  Statistics of the output (stats_out:
    // part-major with stride M) are not emitted by a split problem: the caller gets INSV2V_EUNSUPPORTED and takes the statistics pass.
    if (split) {
        if (d.batch > 1 || d.stats_out || d.split_k > 1) return refuse(INSV2V_EUNSUPPORTED);
        const int64_t per = units_per_part(d, window), total = conv ? d.NB : d.M;
        if (per <= 0) return refuse(INSV2V_EUNSUPPORTED);
        const bool finalize = d.stats_parts > 0;   // partial row statistics are finalised over the whole problem first
        if (finalize) stats_finished(d);
        const insv2v_gemm_plan_t first = plan_gemm(window_part(d, 0, per), cus, window, sw);   // (the last part may be smaller: planned when it runs)
        if (first.rc) return refuse(first.rc);
        const int32_t stats_w_ = p.stats_width, fuse = p.gn_fuse;
        p = first;
        p.stats_width = stats_w_; p.gn_fuse = fuse; p.ln_finalize = finalize;
        p.parts = (int32_t)((total + per - 1) / per);
        p.units_per_part = (int32_t)per;
        return p;
    }
    if (d.w_group_rows > 0) {   // grouped weights (validated above): gemm_r8 / gemm_q8 by the rounds of tiles each needs
        const int64_t groups = ((int64_t)d.M + d.w_group_rows - 1) / d.w_group_rows;
        if (beyond_2g(groups * d.w_group_stride * 2)) return refuse(INSV2V_EUNSUPPORTED);
        if (cus <= 0) return refuse(INSV2V_EINVAL);
        const bool r_ok = d.N % 320 == 0, q_ok = d.N % 256 == 0;
        const pingpong_cost c = pingpong_costs(d, cus);
        const bool use_r = d.tile / 10 == 24 ? true : d.tile / 10 == 23 ? false : (r_ok && (!q_ok || c.r8 <= c.q8));
        if (use_r ? !r_ok : !q_ok) return refuse(INSV2V_EUNSUPPORTED);
        if (const int rc = engine(use_r ? R8 : Q8)) return refuse(rc);
        return p;
    }
    // forced tile codes: 1-9 (+10 x ring depth) the tile kernel, 100-103 the patch-tiled kernel's configurations, 210-221 gemm_w4,
    // 230-239 gemm_q8, 240-249 gemm_r8 (the last digits: the engine's variant)
    if (d.tile >= 200 && d.tile <= 206) return refuse(INSV2V_EUNSUPPORTED);   // round 3's 256x256 kernel (gemm_p8): retired in round 6, source kept under tools/archive/
    if ((d.tile >= 230 && d.tile <= 249) || (d.tile >= 210 && d.tile <= 221)) {
        const int family = d.tile >= 240 ? R8 : d.tile >= 230 ? Q8 : W4;
        if (d.split_k > 1 || (d.stats_out && family != R8)) return refuse(INSV2V_EUNSUPPORTED);
        d.split_k = 1;
        if (const int rc = engine(family, d.tile - engine_tile_code(family))) return refuse(rc);
        return p;
    }
    const int nsplit = d.stats_out ? 1 : split_choice(d);
    int shape = d.tile % 10, ring = d.tile / 10;   // tile code: low digit = tile shape (0 auto), tens digit = ring depth (0 default = 2, or 2 / 3 / 4)
    if (nsplit > 1) splitk_main_pass(d, nsplit);
    else d.split_k = 1;
    if (nsplit > 1 && shape == 0) shape = 5;
    const bool by_rule = nsplit <= 1 && d.tile == 0;
    if (by_rule && !d.gn_ab) {   // (with stats_out: gemm_r8 or nothing)
        const int pp = pingpong_choice(d, d.stats_out != nullptr, cus, sw);
        if (pp && !engine(pp == 2 ? R8 : Q8)) return p;
        // (a statistics buffer sized for gemm_r8's 160-column parts must not reach a kernel with another part width)
        if (pp && d.stats_out) return refuse(INSV2V_EUNSUPPORTED);
    }
    // Round 4: the GEGLU FF1 of levels 1-3 (N = 5120 / 10240 = whole 320-row tiles) on the 256x320 kernel where its rounds of tiles
    // cost no more than the 256x256 kernel's: 7 % faster at K = 640, 3.5 % at K = 1280 (profiles/r04_gemm_r8_geglu.txt)
    if (by_rule && !d.stats_out && d.act == INSV2V_ACT_GEGLU && !conv && !d.k_split && !d.residual && sw.r8_geglu && cus > 0 && d.N % 320 == 0 &&
        d.M >= 8192 && d.K >= 640 && !d.c_fp32 && d.batch <= 1) {
        const pingpong_cost c = pingpong_costs(d, cus);
        if (c.r8 <= c.q8 && !engine(R8)) return p;
    }
    if (by_rule && !d.stats_out) {
        const int pick = persistent_choice(d, sw);
        if (pick && !engine(pick == 1 ? Q8 : W4)) return p;
    }
    if (nsplit <= 1 && (d.tile == 100 || d.tile == 0)) {
        const int tws = halo_tw_shift(d);
        if (d.tile == 100 && (tws < 0 || d.act >= INSV2V_ACT_RELU)) return refuse(INSV2V_EUNSUPPORTED);
        if (tws >= 0 && d.act < INSV2V_ACT_RELU && (d.tile == 100 || halo_fills_chip(d))) return halo(0, tws);
    }
    if (d.gn_ab) return refuse(INSV2V_EUNSUPPORTED);   // only the patch-tiled kernel's product form normalises its input (never silently skip the norm)
    // Round 3: convolutions the patch kernel cannot tile (8x12 / 4x6 latents, stride 2) at the stacked-clip sizes: the 256x256 persistent
    // kernel beats the gathered 128x128 tile once M fills it (23 040 x 1 280 x 11 520: 712 vs 838 us, x 23 040: 1 357 vs 1 597 us;
    // at M = 4 608 it loses 340 vs 192 us, at M = 5 760 320 vs 206 us, at M = 11 520 (10 stacked clips at the 4x6 level) it wins 330 vs 384 us -
    // tools/bench_conv_tiles_r03.py, profiles/r03_conv_tile_sweep_stacked.txt, r03_conv_tile_sweep_B30.txt)
    // (partial row statistics are not finalised on this path: no convolution folds a LayerNorm)
    if (by_rule && conv && d.batch == 1 && !d.c_fp32 && d.M >= 10240 && d.N >= 640 && d.K >= 5760 && sw.persistent && !engine(Q8, 0, false)) return p;
    if (d.tile >= 101 && d.tile <= 103) {   // the patch-tiled kernel's A/B configurations, forced only: 101 = the K-group variant, 102 = 4 waves with
        int tws = halo_tw_shift(d);          // 64 x 64 wave tiles, 103 = ONE 16-wave workgroup per CU on a 256-pixel patch (16 x 16 or 32 x 8)
        if (d.act >= INSV2V_ACT_RELU || (nsplit <= 1 && tws < 0)) return refuse(INSV2V_EUNSUPPORTED);
        if (d.tile == 103) tws = (d.OH % 16 == 0 && d.OW % 16 == 0) ? 4 : (d.OH % 32 == 0 && d.OW % 8 == 0) ? 3 : -1;
        if (nsplit <= 1) return tws < 0 ? refuse(INSV2V_EUNSUPPORTED) : halo(d.tile - 100, tws);
    }
    if (shape == 0) shape = pick_tile(d);
    if (d.act == INSV2V_ACT_GEGLU && tile_bn(shape) == 64) shape = 2;
    if (ring == 0) ring = 2;
    if (ring < 2 || ring > 4 || shape < 1 || shape > 9) return refuse(INSV2V_EINVAL);
    if (tile_lds_bytes(tile_bm(shape), tile_bn(shape), ring) > TILE_LDS_MAX) return refuse(INSV2V_EUNSUPPORTED);
    p.family = INSV2V_PLAN_TILE; p.variant = shape; p.ring = ring; p.forced_tile = shape + 10 * ring;
    p.split_k = nsplit; p.splitk_reduce = nsplit > 1;
    return p;
}
