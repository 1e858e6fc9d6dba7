// Register-resident row kernels for the C = 320 / 640 levels of the UNet: what csrc/rows_ffn.hip (feed-forward + row Linear),
// csrc/rows_tattn.hip (temporal attention) and csrc/rows_xattn.hip (text cross-attention) share.  The kernels:
//   insv2v_ffn_fused   out = x + W2 . ( h * gelu_erf(g) ) + b2,  [h; g] = W1 . LayerNorm(x) + b1  [-> proj_out + residual]   (C = 320)
//   insv2v_rowlin      out = [LayerNorm | GroupNorm](x) . W^T + bias | per-frame bias [+ residual]        (every K = 320 / 640 Linear)
//   insv2v_tattn_fused one temporal attention sub-block incl. to_out + residual (C = 320);  insv2v_tattn_attn: up to the attention output (C = 640)
//   insv2v_xattn_fused one text cross-attention sub-block incl. to_out + residual (C = 320); insv2v_xattn_attn: up to the attention output (C = 640)
// (diffusers FeedForward(geglu) behind norm3 / ff_norm: attention.py:259, motion_module.py:214; the Linear / 1x1-conv layers of
// attention.py:64,89,160-190 and motion_module.py:139,146,289-331 at the 320-channel level.)
//
// Why: at K = 320 a tile of the ordinary GEMM kernels spends as long in its prologue and global epilogue as in its five K slices
// (330-700 TFLOP/s), and the feed-forward writes and re-reads a 73 728 x 1 280 hidden tensor.  Here the
// activations never leave the register file:
//   * a wave owns 32 tokens; their 320 (normalised) channels sit in 80 VGPRs as MFMA B-operand fragments, loaded once;
//     LayerNorm statistics = in-lane sums + one cross-lane exchange (no statistics pass, no folded-LayerNorm epilogue);
//   * every weight fragment (A operand of one v_mfma_f32_32x32x16_f16: 64 lanes x 16 B = 1 KiB) comes from ONE linear fp16 stream
//     laid out on the host in exactly the order the MFMAs consume it, brought in by LDS-DMA through a ring of slots shared by the 4
//     waves of a workgroup (128 tokens, one workgroup per CU, persistent over row tiles); a fragment read is a conflict-free
//     ds_read_b128 at lane x 16; fragments are read 8 at a time, one group ahead of the MFMAs that use them;
//   * biases ride in one extra k-step against a constant fragment (ones, or the one-hot of the token's frame for the temporal
//     positional-encoding table) - no bias tables, no epilogue arithmetic;
//   * feed-forward: the hidden layer is walked in chunks of 32 units: S = W1_chunk . x (2 x 21 MFMAs), GEGLU in registers, and the
//     fp16 result IS the B operand of the second contraction O += W2_chunk . P (20 MFMAs into 160 accumulator registers): the C
//     layout of one MFMA and the B layout of the next differ only by a permutation of k that is applied to the weights on the host
//     (insv2v/fused.py).  GEGLU of chunk k is issued between the MFMAs of S for chunk k+1 (two S buffers).
// One wave per SIMD (up to 512 registers): nothing overlaps a wave's MFMAs but its own instruction stream, and measured on MI355X
// every non-MFMA instruction costs ~6 cycles that do not hide (profiles/r03_ffn_fused_ablation.txt) - hence one s_waitcnt per
// fragment group, scalar-only ring bookkeeping and 32 KiB slots (one barrier per 32 MFMAs) in the feed-forward.
// Roofline: MFMA; HBM traffic = x once in, out once out + the L2-resident weight stream.
#pragma once
#include "common.h"
#include "gemm_dma.h"
#include <type_traits>
#include <utility>

namespace {
template <int V> using ic = std::integral_constant<int, V>;

constexpr int FC = 320;                 // channels
constexpr int KS1 = FC / 16;            // 20 k-steps over the channels (+1 bias step)

__device__ __forceinline__ unsigned pk2(float a, float b) {
    const half2v h = {(half_t)a, (half_t)b};
    return __builtin_bit_cast(unsigned, h);
}

typedef unsigned uint4v __attribute__((ext_vector_type(4)));

// ---- the weight ring.  Stream slot q (PASS_SLOTS per pass over the weights, wrapping) lives in ring slot q % NS; a slot is SLOT_FR
// fragments; wave w requests pieces w*PPS .. w*PPS+PPS-1 (1 KiB each) of every slot.  Requests run NS-1 slots ahead of the reads.
// Fragments are consumed in groups of 8, one group BEHIND their read, and every consumed group requests 2 pieces: when slot q is
// acquired, everything up to slot q + NS - 2 has been requested except the 2 pieces attached to the group consumed after the
// acquire, so slot q has landed once at most PPS (NS - 2) - 2 pieces are outstanding (loads and stores of a wave retire in issue
// order, so other memory operations in between only make this wait conservative).  All bookkeeping is wave-uniform (SALU).
// The two-source rings of the text cross-attention kernels (rows_xattn.hip) derive from Ring for its LDS side: state, advance_lds, acquire
// and read_group.
template <int SLOT_FR_, int NS_, int GS_ = 8>
struct Ring {
    // GS = fragments per read / consume group (8, or 4 where a fragment feeds two MFMAs and 32 registers of read-ahead are enough);
    // a consumed group requests PPG = GS / 4 pieces
    static constexpr int SLOT_FR = SLOT_FR_, NS = NS_, GS = GS_, SLOT_B = SLOT_FR_ * 1024, PPS = SLOT_FR_ / 4, GPS = SLOT_FR_ / GS_, PPG = GS_ / 4;
    static_assert(PPS == PPG * GPS && (GS_ == 8 || GS_ == 4), "whole pieces per fragment group");
    char* smem;
    srd_t rW;
    unsigned lane16;
    int iss_lds, iss_soff, pass_bytes, wave_off, rd_off;   // byte offsets (wave-uniform)
    const char* rd;                                          // this lane's view of the slot being read

    __device__ __forceinline__ void init(char* smem_, const void* stream, int pass_slots, int wid, int lane) {
        smem = smem_;
        rW = make_srd(stream);
        lane16 = (unsigned)(lane * 16);
        wave_off = wid * PPS * 1024;
        iss_lds = 0; iss_soff = 0;
        pass_bytes = pass_slots * SLOT_B;
        rd_off = (NS - 1) * SLOT_B;
        rd = smem_;
#pragma unroll 1
        for (int s = 0; s < NS - 1; ++s) {
            pieces<0, PPS>();
            advance();
        }
    }
    // piece I of the slot being requested: pieces 0 .. 3 / 4 .. 7 share one scalar offset and one LDS base (M0), the KiB inside rides in the
    // instruction's immediate offset (added to both addresses): two scalar operations per request less
    template <int I>
    __device__ __forceinline__ void piece() {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rW, (__attribute__((address_space(3))) void*)(smem + iss_lds + wave_off + (I >> 2) * 4096), 16, lane16,
                                                 iss_soff + wave_off + (I >> 2) * 4096, (I & 3) * 1024, 0);
    }
    template <int I0, int N>
    __device__ __forceinline__ void pieces() {
        if constexpr (N > 0) { piece<I0>(); pieces<I0 + 1, N - 1>(); }
    }
    __device__ __forceinline__ void advance_lds() { iss_lds = iss_lds + SLOT_B == NS * SLOT_B ? 0 : iss_lds + SLOT_B; }
    __device__ __forceinline__ void advance() {
        advance_lds();
        iss_soff = iss_soff + SLOT_B == pass_bytes ? 0 : iss_soff + SLOT_B;
    }
    // piece `which` (0 .. PPG-1) of consumption phase ph (= consumed-group index mod GPS)
    template <int PH, int WHICH>
    __device__ __forceinline__ void refill() {
        piece<PPG * PH + WHICH>();
        if (WHICH == PPG - 1 && PH == GPS - 1) advance();
    }
    __device__ __forceinline__ void acquire() {
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(PPS * (NS - 2) - PPG) : "memory");  // own pieces landed; own reads of older slots returned
        __builtin_amdgcn_s_barrier();   // everyone's pieces are in LDS; everyone is done with the previous slot
        asm volatile("" ::: "memory");
        rd_off = rd_off + SLOT_B == NS * SLOT_B ? 0 : rd_off + SLOT_B;
        rd = smem + rd_off + lane16;
    }
    __device__ __forceinline__ half8 frag(int i) const { return *(const half8*)(rd + i * 1024); }
    // group g of a section (sections start on a slot boundary) -> register buffer; acquires the slot at its first group
    template <int G>
    __device__ __forceinline__ void read_group(half8 (&fb)[GS_]) {
        if (G % GPS == 0) acquire();
#pragma unroll
        for (int i = 0; i < GS; ++i) fb[i] = frag((G % GPS) * GS + i);
        // keep the reads together, ahead of the MFMAs of the previous group
        __builtin_amdgcn_sched_barrier(0);
    }
};

__device__ __forceinline__ void zero16(floatx16& a) {
#pragma unroll
    for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

// LayerNorm (no affine: gamma / beta live in the weights) of a token's channels held as natural-order fragments, in place:
// statistics = in-lane sums + one exchange with the other lane half
template <int KS>
__device__ __forceinline__ void layernorm_frags(half8 (&xf)[KS], float eps) {
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) sum += (float)xf[s][e];
    sum += __shfl_xor(sum, 32, 64);
    const float mean = sum * (1.f / (16 * KS));
    // (opaque re-definitions between the three passes: otherwise hipcc keeps all 16 KS converted floats alive next to the packed
    //  halfs - 480 registers per 32-token block at K = 640 - instead of converting again)
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(xf[s]));
    float var = 0.f;
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) { const float d = (float)xf[s][e] - mean; var = fmaf(d, d, var); }
    var += __shfl_xor(var, 32, 64);
    const float rstd = rsqrtf(var * (1.f / (16 * KS)) + eps);
#pragma unroll
    for (int s = 0; s < KS; ++s) asm volatile("" : "+v"(xf[s]));
#pragma unroll
    for (int s = 0; s < KS; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) xf[s][e] = (half_t)(((float)xf[s][e] - mean) * rstd);
}

// ---- this lane's channels of its token as B-operand fragments, 16 bytes per load: k-step s, slots 0-7 = channels 16 s + 8 half .. +7
// (the "natural" k order: fused.py packs the weights of a layer that reads its input from memory with it; layers that consume an
// MFMA result in registers use the C-layout order instead).  request_rows only issues the loads (the row Linear requests the NEXT tile's
// rows before its last epilogue); load_rows optionally LayerNorms them.
template <int KS>
__device__ __forceinline__ void request_rows(half8 (&xf)[KS], srd_t rX, unsigned xoff) {
#pragma unroll
    for (int s = 0; s < KS; ++s) xf[s] = __builtin_bit_cast(half8, (uint4v)__builtin_amdgcn_raw_buffer_load_b128(rX, xoff, s * 32, 0));
}
template <int KS, bool LN>
__device__ __forceinline__ void load_rows(half8 (&xf)[KS], srd_t rX, unsigned xoff, float eps) {
    request_rows<KS>(xf, rX, xoff);
    if (LN) layernorm_frags<KS>(xf, eps);
}

// ---- one 32-channel accumulator tile -> memory, 16 bytes per lane and store.  In the MFMA C layout lane (token, half) owns channels
// 8 q + 4 half .. +3 of register quad q; v_permlane32_swap exchanges quad 2j+1 of the lower lane half with quad 2j of the upper one,
// after which the lower lane holds channels 16 j .. 16 j + 7 and the upper lane 16 j + 8 .. + 15 of its token: two 16-byte stores
// per tile instead of four 8-byte ones (row-scattered 8-byte stores are store-issue bound at ~7 B/clk/CU - this kernel's first
// version spent most of its time there).  The optional residual arrives by 16-byte loads in the same layout and is added in fp32.
// off = byte offset of (token row, channel 8 half) or OOB; soff0 = byte offset of the tile's first channel.
template <bool RES>
__device__ __forceinline__ void load_res_tile(uint4v (&rv)[2], srd_t rR, unsigned off, int soff0) {
    if (!RES) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) rv[j] = (uint4v)__builtin_amdgcn_raw_buffer_load_b128(rR, off, soff0 + j * 32, 0);
}
// Two fp32 values (+ the two fp16 residual values of one dword) -> one packed fp16 dword: v_fma_mixlo / mixhi_f16 (acc * 1.0 + residual
// half, fp32 arithmetic, one rounding to fp16 - the values of convert + add + convert-pack, in 2 instructions per pair instead of 5;
// profiles/r05_rows_epilogue_mix_dot2.txt).
__device__ __forceinline__ unsigned pack_res2(float a, float b, unsigned res) {
    unsigned d;
    asm("v_fma_mixlo_f16 %0, %1, 1.0, %2 op_sel_hi:[0,0,1]" : "=v"(d) : "v"(a), "v"(res));
    asm("v_fma_mixhi_f16 %0, %1, 1.0, %2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(d) : "v"(b), "v"(res));
    return d;
}
// (sum x, sum x^2) of the two fp16 values of a packed dword, fp32 accumulation: two v_dot2_f32_f16 instead of 2 converts + 2 adds + 2 FMAs
__device__ __forceinline__ void stats2(unsigned o, float& s1, float& s2) {
    typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
    const f16x2 v = __builtin_bit_cast(f16x2, o), one = {(_Float16)1.f, (_Float16)1.f};
    s1 = __builtin_amdgcn_fdot2(v, one, s1, false);
    s2 = __builtin_amdgcn_fdot2(v, v, s2, false);
}
// 16-byte chunk j (0 / 1) of an accumulator tile (+ its residual chunk): channels 16 j + 8 half .. + 7 of the lane's token, packed to fp16
template <bool RES>
__device__ __forceinline__ uint4v tile_chunk(const floatx16& acc, const uint4v& rvj, int j) {
    float v[8];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        // (scalars first: __builtin_bit_cast applied directly to a vector subscript takes element 0 with this hipcc, ROCm 7.2)
        const float alo = acc[8 * j + e], ahi = acc[8 * j + 4 + e];
        const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, alo), __builtin_bit_cast(unsigned, ahi), false, false);
        const unsigned lo = r[0], hi = r[1];
        v[e] = __builtin_bit_cast(float, lo);
        v[4 + e] = __builtin_bit_cast(float, hi);
    }
    uint4v o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned rk = rvj[k];
        o[k] = RES ? pack_res2(v[2 * k], v[2 * k + 1], rk) : pk2(v[2 * k], v[2 * k + 1]);
    }
    return o;
}
template <bool RES>
__device__ __forceinline__ void store_tile(const floatx16& acc, const uint4v (&rv)[2], srd_t rO, unsigned off, int soff0, float* s1 = nullptr, float* s2 = nullptr) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint4v o = tile_chunk<RES>(acc, rv[j], j);
        if (s1) {   // LayerNorm statistics of the NEXT op, from the fp16 values being stored
#pragma unroll
            for (int k = 0; k < 4; ++k) { const unsigned ok = o[k]; stats2(ok, *s1, *s2); }
        }
        __builtin_amdgcn_raw_buffer_store_b128(o, rO, off, soff0 + j * 32, 0);
        // Keep the store's data registers untouched for a few cycles: with a second wave on the SIMD (two row-linear workgroups per
        // CU) a 16-byte store still reads part of its data when the next VALU instruction reuses the registers - the hazard found
        // in round 2 (profiles/r02_gemm_debug.md); here it showed as NaNs in the M = 73 733 test.  The "v" input pins them.
        asm volatile("s_nop 7" ::"v"(o));
    }
}
// store_tile without the store: chunk j is exactly the natural-order B fragment of k-step 2 t + j of a following contraction
template <bool RES>
__device__ __forceinline__ void finish_tile(const floatx16& acc, const uint4v (&rv)[2], half8 (&out)[2]) {
#pragma unroll
    for (int j = 0; j < 2; ++j) out[j] = __builtin_bit_cast(half8, tile_chunk<RES>(acc, rv[j], j));
}

template <int... I, class Fn>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, I...>, Fn&& f) { (f(ic<I>{}), ...); }
template <int N, class Fn>
__device__ __forceinline__ void static_for(Fn&& f) { static_for_impl(std::make_integer_sequence<int, N>{}, f); }

__device__ __forceinline__ void pack_tile(const floatx16& a, half8& k0, half8& k1) {   // C layout -> the two operand fragments (k-steps)
    const uint4v u0 = {pk2(a[0], a[1]), pk2(a[2], a[3]), pk2(a[4], a[5]), pk2(a[6], a[7])};
    const uint4v u1 = {pk2(a[8], a[9]), pk2(a[10], a[11]), pk2(a[12], a[13]), pk2(a[14], a[15])};
    k0 = __builtin_bit_cast(half8, u0);
    k1 = __builtin_bit_cast(half8, u1);
}

// ---- constant B fragments of a bias k-step.  bias_ones: k-slots 0 and 1 of the lower lane half are 1 (bias hi + lo parts).
// frame_hot: the one-hot of the token's frame fr against a per-frame table, for the lane half that holds frames 8 oct .. 8 oct + 7
__device__ __forceinline__ half8 bias_ones(int half) {
    half8 ones = {0, 0, 0, 0, 0, 0, 0, 0};
    if (half == 0) { ones[0] = (half_t)1.f; ones[1] = (half_t)1.f; }
    return ones;
}
__device__ __forceinline__ half8 frame_hot(int fr, int oct) {
    half8 f;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = (oct == (fr >> 3) && e == (fr & 7)) ? (half_t)1.f : (half_t)0.f;
    return f;
}

int num_cus() { return insv2v_num_cus(); }

// Operands beyond one 2 GiB descriptor.  The fused kernels address x / out / residual through descriptors built at the operand's base, with
// 32-bit lane offsets.  Their launchers run a problem whose operands reach beyond the window as RANGES OF WHOLE UNITS - 128-row tiles
// (feed-forward), samples (temporal and text attention: a wave / a tile never reads across a sample) - one launch per range with the base
// pointers advanced on the host, as insv2v_gemm does for row / image ranges.  The kernels do not know: an in-window problem is one launch,
// exactly as before, and a row's arithmetic does not depend on the range it falls in.  unit_bytes = the widest operand's bytes per unit;
// a unit that does not fit by itself is refused; whole_bytes = the widest operand's extent where the last unit is partial.  launch(u0, nu)
// launches units [u0, u0 + nu).  The window is the hardware's 2^31 bytes unless a test shrank it (insv2v_set_operand_window), so that
// small problems can take this path.
template <class Fn>
int launch_unit_ranges(int64_t units, int64_t unit_bytes, Fn&& launch, int64_t whole_bytes = -1) {
    const int64_t ov = insv2v_operand_window_override(), lim = ov > 0 ? ov : (int64_t)1 << 31;
    if (units <= 0 || unit_bytes <= 0 || unit_bytes >= lim) return INSV2V_EUNSUPPORTED;
    if ((whole_bytes >= 0 ? whole_bytes : units * unit_bytes) < lim) return launch((int64_t)0, units);
    int64_t per = (lim - 1) / unit_bytes;
    const int64_t nparts = (units + per - 1) / per;
    per = (units + nparts - 1) / nparts;   // parts as even as possible
    for (int64_t u0 = 0; u0 < units; u0 += per) {
        const int rc = launch(u0, units - u0 < per ? units - u0 : per);
        if (rc != 0) return rc;
    }
    return 0;
}

// `grid` persistent workgroups of 256 threads with `lds` bytes of dynamic LDS
template <class Args>
int launch_grid(const void* kernel, bool& attr_set, int lds, const Args& args, int grid, hipStream_t s) {
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return (int)e;
        attr_set = true;
    }
    if (grid <= 0) return INSV2V_EINVAL;
    Args a = args;
    void* kargs[] = {&a};
    hipError_t le = hipLaunchKernel(kernel, dim3(grid), dim3(256), kargs, lds, s);
    if (le != hipSuccess) return (int)le;
    return launch_status();
}

// one workgroup per 128-row tile of M rows, at most wgs_per_cu per CU
template <class Args>
int launch_rows(const void* kernel, bool& attr_set, int lds, const Args& args, int M, hipStream_t s, int wgs_per_cu = 1) {
    const int ncu = num_cus() * wgs_per_cu;
    const int ntiles = (M + 127) / 128;
    return launch_grid(kernel, attr_set, lds, args, ntiles < ncu ? ntiles : ncu, s);   // (no CU count: grid <= 0 is refused there)
}

}  // namespace
