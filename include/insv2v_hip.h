/*
 * insv2v_hip.h -- C ABI of libinsv2v_hip.so: the MI355X (gfx950) kernels behind the
 * InsV2V denoising hot path.
 *
 * The reference (amazon-science/instruct-video-to-video) is pure Python/PyTorch and has no
 * FFI layer; the seam is the set of library ops its hot path dispatches.
 * Each entry point below replaces those ops for one stage of the path and cites the reference
 * call sites it stands in for (file:line relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is allocated inside;
 *   - activations are fp16, channels-last: a video tensor (b,c,f,h,w) is stored as the token
 *     matrix [b*f*h*w, c]; weights are fp16 [out, in] (conv: [out, kh, kw, in]); biases,
 *     norm affine parameters and statistics are fp32;
 *   - all sizes are element counts, all strides are in elements;
 *   - return value 0 = launched, negative = rejected argument (INSV2V_E*), positive = hipError_t;
 *   - launches are asynchronous on `stream` and re-entrant per stream (graph-capturable);
 *   - one process drives ONE device (the deployment is one process per GPU): the launchers cache the CU count and kernel
 *     attributes of the first device they run on, and a call made with another device current returns INSV2V_EINVAL.
 */
#ifndef INSV2V_HIP_H
#define INSV2V_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* insv2v_stream_t; /* hipStream_t */

#define INSV2V_OK 0
#define INSV2V_EINVAL (-1)  /* bad shape / alignment / null pointer */
#define INSV2V_EUNSUPPORTED (-2)

#define INSV2V_ACT_NONE 0
#define INSV2V_ACT_SILU 1
#define INSV2V_ACT_GEGLU 2 /* W rows interleaved [h0..31,g0..31,h32..63,...]; out has N/2 columns */
#define INSV2V_ACT_QUICK_GELU 3 /* x * sigmoid(1.702 x): CLIP text MLP (transformers modeling_clip CLIPMLP, hidden_act "quick_gelu") */

/* activations of the optical-flow estimator's convolutions (torchvision raft_large behind flow_utils.py:134-189: ReLU after every
 * Conv2dNormActivation, sigmoid / tanh in the ConvGRU); insv2v_gemm LINEAR mode and, since round 6, CONV3X3 mode on the 128x128 tile kernel (the 3x3 layers of that network without im2col) */
#define INSV2V_ACT_RELU 4
#define INSV2V_ACT_SIGMOID 5
#define INSV2V_ACT_TANH 6

#define INSV2V_MODE_LINEAR 0
#define INSV2V_MODE_CONV3X3 1

/* ABI version, bumped on any struct change.
 * ABI 14: seeded noise - insv2v_randn, insv2v_posterior_sample_seeded and the noise_seed / noise_stream / noise_on fields of
 * insv2v_step_desc (section "seeded noise" below holds the stream definition, which is part of this contract).
 * ABI 15: insv2v_groupnorm_plan (an addition: no existing struct or entry changes); likewise the CLIP scoring entries
 * (insv2v_clip_preprocess, insv2v_clip_scores, insv2v_l2_normalize) and the pixel-space scores (insv2v_warp_error,
 * insv2v_frame_fidelity and their workspace queries), added without a bump. */
int insv2v_abi_version(void);
/* One-time per-process setup (kernel attributes). Safe to call repeatedly. */
int insv2v_init(void);

/*
 * insv2v_gemm: C = epilogue(alpha * A x W^T), MFMA fp16 -> fp32 accumulate.
 *
 * LINEAR mode: A is [M,K] (row stride lda). If k_split > 0, columns [0,k_split) come from `a`
 *   and [k_split,K) from `a2` (row stride lda2): a channel concat that is never materialised.
 *   Replaces torch.nn.Linear / 1x1 Conv2d at attention.py:64,89 (proj_in/out), resnet.py:172,200
 *   (conv_shortcut), resnet.py:183 (time_emb_proj), unet.py:358-364 (TimestepEmbedding),
 *   motion_module.py:139,146, diffusers Attention.to_q/k/v/to_out and FeedForward
 *   (attention.py:160-190, motion_module.py:200,289-331), vqvae/model.py:149-172 (VAE attn 1x1).
 * CONV3X3 mode: implicit GEMM of a 3x3 convolution over an NHWC image [NB,IH,IW,*]:
 *   M = NB*OH*OW, K = 9*Cin, W is [N, 3,3,Cin]. Input pixel for output (oh,ow), tap (kh,kw) is
 *   (oh*stride+kh-pad_t, ow*stride+kw-pad_l), zero outside; with upsample=1 the input is first
 *   nearest-x2 upsampled (index>>1) without materialising it. Channel concat via k_split (=C1).
 *   (ABI 13) upsample=1 is valid only with stride = 1, pad_t = pad_l = 1 and OH in {2*IH-1, 2*IH}, OW in {2*IW-1, 2*IW}
 *   (anything else: INSV2V_EINVAL).  OH x OW is the extent of the upsampled image: 2*IH-1 / 2*IW-1 is the x2 image WITHOUT its
 *   last row / column (F.interpolate(size=..., mode="nearest") for those sizes, Upsample3D's output_size, resnet.py:41-61) and the
 *   zero padding sits at that cropped edge - not "convolve the x2 image, then crop".  The patch-tiled kernel takes exact x2 only.
 *   Cin must be a multiple of 64 (pad channels on the host) and k_split a multiple of 64.
 *   Replaces F.conv2d at resnet.py:10-18 (InflatedConv3d), :59-69 (Upsample3D), :87-105
 *   (Downsample3D), unet.py:92,225 and vqvae/model.py:35-74,77-136 (VAE convs incl. the
 *   asymmetric (0,1,0,1) pad of Downsample: pad_t=pad_l=0, stride=2).
 * Epilogue (in this order): v = alpha*acc; [folded LayerNorm, see below]; += bias[n];
 *   += row_bias[g*ld_rb + n] with g = m / rows_per_group (the per-sample time embedding add of
 *   resnet.py:183-186), or g = (m / rows_per_group) % rb_mod when rb_mod > 0 (per-frame term);
 *   act (SiLU, or GEGLU h*gelu_erf(g)); += residual[m*ldr + n]; store fp16 (or fp32 if c_fp32).
 * Folded LayerNorm (row_stats != NULL): the GEMM consumes the RAW tokens x while computing
 *   LayerNorm(x) W^T:  with W' = W*diag(gamma) passed as `w`, col_sum[n] = sum_k W'[n,k] and
 *   row_stats[m] = (mean_m, rstd_m) from insv2v_layernorm_stats,
 *       v = rstd_m * (alpha*acc - mean_m * col_sum[n])          (= ((x-mean)*rstd*gamma) . W[n,:])
 *   the beta term (sum_k beta_k W[n,k]) is folded into `bias` by the caller, and the temporal positional
 *   encoding added after the norm (motion_module.py:277-278) becomes the per-frame row_bias table
 *   pe @ W^T.  Removes the normalised copy of the activations from HBM (attention.py:236-259,
 *   motion_module.py:206,214).
 * Batched: grid y = batch, operands advanced by *_bs elements per batch.  With k_split > 0 the second source `a2` advances by a_bs
 *   elements too (there is no stride of its own), whatever lda2 is: its batches lie a_bs elements apart.
 * Split-K: when `workspace` is given (fp32 scratch of workspace_bytes) the library may split K over
 *   split_k workgroups per tile (0 = decide automatically: only for problems too small to fill the GPU
 *   with long K, e.g. the 4x6-latent UNet level) and reduce the fp32 partials in a second kernel that
 *   applies the epilogue; results are deterministic (fixed summation order).
 */
typedef struct insv2v_gemm_desc {
    const void* a;
    const void* a2;
    const void* w;
    void* c;
    const float* bias;
    const float* row_bias;
    const void* residual;
    const float* row_stats; /* [M][2] (mean, rstd) or NULL */
    const float* col_sum;   /* [N] or NULL (required with row_stats) */
    int64_t lda, lda2, ldw, ldc, ldr, ld_rb;
    int64_t a_bs, w_bs, c_bs, r_bs;
    void* workspace;
    int64_t workspace_bytes;
    int32_t M, N, K;
    int32_t k_split;
    int32_t rows_per_group;
    int32_t rb_mod;
    int32_t act;
    int32_t c_fp32;
    int32_t mode;
    int32_t NB, IH, IW, OH, OW, Cin;
    int32_t stride, pad_t, pad_l, upsample;
    int32_t batch;
    int32_t tile; /* 0 = auto; low digit = tile shape, tens digit = LDS ring depth (tools/bench_gemm.py) */
    int32_t split_k; /* 0 = auto (needs workspace), 1 = never, S > 1 = force */
    float alpha;
    /* Fused input GroupNorm (+SiLU) of ResnetBlock3D (resnet.py:177-178,188-194), CONV3X3 mode on the patch-tiled kernel
     * only: the convolution reads the RAW tensor and applies y = act(x*scale + shift) to its input patch in LDS, so the
     * normalised copy never exists in HBM.  gn_ab = [nsamples][Cin][2] fp32 (scale, shift) from insv2v_groupnorm
     * (stats_only); image nb belongs to sample nb / gn_images_per_sample.  Zero padding stays zero.  A call that sets gn_ab
     * but cannot run on the patch-tiled kernel is rejected (INSV2V_EUNSUPPORTED), never silently un-normalised: ask
     * insv2v_conv3x3_fuses_groupnorm first. */
    const float* gn_ab;
    int32_t gn_images_per_sample;
    int32_t gn_silu;
    /* LayerNorm statistics from the PRODUCER instead of a re-read (attention.py:236-259, motion_module.py:206,214: every
     * LayerNorm input is the output of an N = C GEMM).  stats_out != NULL (LINEAR mode, fp16 output): the epilogue also writes,
     * per output row and per column tile tn of insv2v_gemm_stats_parts() tiles, the partial sums (sum v, sum v^2) of the
     * values it stores (128x128 tile: after the fp16 rounding; 256x320 ping-pong tile, 160-column parts: before it):
     * stats_out[(tn*M + m)*2 + {0,1}] fp32 (tile-major, deterministic).  A consumer passes that buffer as
     * row_stats with stats_parts = number of tiles (0 = row_stats already holds (mean, rstd)) and ln_eps: it finalises
     * mean = S1/K, rstd = rsqrt(S2/K - mean^2 + eps) itself (K = the LayerNorm width); kernels that need (mean, rstd) pairs get
     * them from a small internal finalize launch into stats_scratch [M][2] (required with stats_parts > 0). */
    float* stats_out;
    float* stats_scratch;
    int32_t stats_parts;
    float ln_eps;
    /* Grouped weights (ABI 11; LINEAR mode on the 256-row ping-pong kernels only): row block g = m / w_group_rows of A / C is multiplied
     * by the weight matrix at w + g * w_group_stride elements (same [N, K] shape and ldw).  w_group_rows must be a multiple of 256 (a tile
     * never straddles two groups); 0 = one weight matrix.  This is the batched product of the Winograd convolution (insv2v_winograd_*:
     * 16 transformed-tap GEMMs as ONE launch); bias / row_bias / residual / statistics / activation are not combined with it. */
    int64_t w_group_stride;
    int32_t w_group_rows;
    int32_t reserved0;
} insv2v_gemm_desc;
int insv2v_gemm(const insv2v_gemm_desc* d, insv2v_stream_t stream);
/* Operand windows (ABI 10).  The kernels address every operand through 32-bit byte offsets inside one 2 GiB buffer descriptor.  A
 * problem whose activations (`a`, `a2`), output or residual reach beyond that window is run by insv2v_gemm as several launches over row
 * ranges (LINEAR) or image ranges (CONV3X3), each inside the window and aligned to the row-bias groups (rows_per_group x rb_mod) and the
 * GroupNorm samples (gn_images_per_sample); partial row statistics (stats_parts > 0) are finalised over the whole problem first.  Such a
 * problem cannot emit stats_out (INSV2V_EUNSUPPORTED, like every problem that cannot), is not batched and takes no forced split-K.
 * insv2v_set_operand_window(bytes) replaces the window size (0 = default: 2 GiB less 1 MiB) and returns the previous value; it exists so
 * that tests can drive small problems through the split path - the product never calls it.
 * The same holds for the fused row kernels, and they obey the same hook: insv2v_ffn_fused, insv2v_tattn_fused / _attn and
 * insv2v_xattn_fused / _attn take x, out, post_residual and pre_residual of any size; a problem beyond one window (2^31 bytes, or the
 * hook's) runs as ranges of whole units, one launch each, bit-identical to one launch.  What has to fit one window is ONE unit of the
 * widest operand (INSV2V_EUNSUPPORTED otherwise, before anything is launched):
 *   insv2v_ffn_fused                      a 128-row tile
 *   insv2v_tattn_fused, insv2v_tattn_attn one sample: frames x HW rows
 *   insv2v_xattn_fused, insv2v_xattn_attn one sample: rows_per_sample rows; and the K / V streams of ALL samples (samples x 176 KiB
 *                                         at C = 320, x 320 KiB at C = 640)
 * insv2v_rowlin (a 256-row tile, or a wave's 32 rows with gn_ab) and insv2v_attention base their descriptors inside the kernel and
 * do not look at the hook.  The Python host restates this arithmetic (insv2v/fused.py check_operand_windows) and refuses a geometry
 * that cannot run before the first launch of a forward. */
int64_t insv2v_set_operand_window(int64_t bytes);
/* Number of column tiles (= partial statistics per row) insv2v_gemm will write for this problem when stats_out is set;
 * 0 if the problem cannot emit statistics (the caller then uses insv2v_layernorm_stats on the output). */
int insv2v_gemm_stats_parts(const insv2v_gemm_desc* d);
/* 1 if insv2v_gemm would run this CONV3X3 problem on the patch-tiled kernel, i.e. accepts gn_ab; else 0. */
int insv2v_conv3x3_fuses_groupnorm(const insv2v_gemm_desc* d);
/* What insv2v_gemm does with a descriptor, without doing it: the answer of the one planner (csrc/gemm_plan.h) that insv2v_gemm,
 * insv2v_gemm_stats_parts and insv2v_conv3x3_fuses_groupnorm all consult.  A pure function of the descriptor's integers, the null /
 * alignment bits of its pointers, the CU count, the operand window in force and the INSV2V_* A/B switches; it touches no GPU.
 * A purely additive entry of ABI 14: no existing struct or entry changes. */
#define INSV2V_PLAN_NONE 0 /* refused (rc != 0) */
#define INSV2V_PLAN_TILE 1 /* gemm_kernel: variant = tile shape 1..9, ring = LDS ring depth 2..4 */
#define INSV2V_PLAN_HALO 2 /* patch-tiled conv_halo_kernel: variant 0 = product, 1..3 = the A/B configurations of tile codes 101..103 */
#define INSV2V_PLAN_Q8 3   /* gemm_q8 256x256, gemm_r8 256x320, gemm_w4 128x256 / 256x128: variant = the engine's variant argument */
#define INSV2V_PLAN_R8 4
#define INSV2V_PLAN_W4 5
typedef struct insv2v_gemm_plan_t {
    int32_t rc;             /* 0, or what insv2v_gemm returns without launching anything (INSV2V_EINVAL / INSV2V_EUNSUPPORTED); with parts > 1 it speaks
                             * for the first part: a smaller last part is planned when it runs and may still be refused */
    int32_t family;         /* INSV2V_PLAN_* */
    int32_t variant;
    int32_t ring;
    int32_t tw_shift;       /* HALO: log2 of the patch width; | 256 with the legacy tile map */
    int32_t cim;            /* R8: the convolution walks K channel-block-major */
    int32_t split_k;        /* split-K factor of the tile kernel, 1 = none */
    int32_t ln_finalize;    /* an ln_finalize launch (partial row statistics -> (mean, rstd)) precedes the kernel */
    int32_t splitk_reduce;  /* a splitk_reduce launch follows it */
    int32_t stats_width;    /* columns per statistics part this problem emits with stats_out set: 0 (cannot), 64, 128 or 160 */
    int32_t gn_fuse;        /* CONV3X3: the kernel this problem runs on with gn_ab set normalises its own input */
    int32_t parts;          /* 1, or the number of in-window parts of a problem beyond the operand window: every part is planned on its own, ... */
    int32_t units_per_part; /* ... of this many rows (LINEAR) / images (CONV3X3), the last maybe fewer; the fields above are the first part's plan */
    int32_t forced_tile;    /* the `tile` code that forces this choice (same split_k, <= 1 for the engines): 1..9 + 10 x ring, 100..103, 210 + variant, 230 + variant, 240 + variant */
} insv2v_gemm_plan_t;
/* cus <= 0: this device's CU count (0 without a GPU: the rules that weigh rounds of tiles then choose nothing).  Returns INSV2V_EINVAL
 * for a NULL argument, else 0 with *out filled - also when out->rc says the problem is refused. */
int insv2v_gemm_plan(const insv2v_gemm_desc* d, int cus, insv2v_gemm_plan_t* out);

/*
 * Winograd F(2x2, 3x3) form of a stride-1, pad-1 3x3 convolution (ResnetBlock3D conv1 / conv2 with wide inputs, resnet.py:143,159 behind
 * InflatedConv3d resnet.py:10-18; ABI 11).  y = A^T [ sum_c (G g G^T) . (B^T d B) ] A per 2x2 output tile: 2.25 x fewer MACs.  Three calls:
 *   insv2v_winograd_input  : x [NB*H*W, C] (channel concat x | x2 at C1; optional GroupNorm scale / shift table gn_ab [nsamples][C][2] as
 *                            from insv2v_groupnorm(stats_only), then SiLU - resnet.py:177-178,188; zero padding applies AFTER the norm)
 *                            -> v = 16 matrices V_k [tiles, C], matrix k = i*4 + j at row offset k * v_group_rows (tiles = NB*ceil(H/2)*ceil(W/2),
 *                            tile order (image, ty, tx); v_group_rows >= tiles, a multiple of 256 for the grouped GEMM)
 *   insv2v_gemm            : a = v [16 * v_group_rows, C], w = U [16][Cout][C] (U_k = (G g G^T)_k, host), w_group_rows = v_group_rows,
 *                            w_group_stride = Cout * C  ->  m [16 * v_group_rows, Cout] fp16
 *   insv2v_winograd_output : m -> y [NB*H*W, Cout] fp16 = A^T M A + bias[Cout] + row_bias[(pixel / rows_per_group) * ld_rb + n]
 *                            (time embedding, resnet.py:183-186) + residual[pixel * ldr + n]
 * H, W of either parity ((ABI 13) odd: the last tile row / column hangs over the image, reads zeros there and stores only the pixels that exist;
 * the upsample form is exact x2 only); C a multiple of 64 (C1 too); W <= 128 (an image's 64-channel slice is staged in LDS whole, or in bands of tile rows with a
 * one-pixel halo); else INSV2V_EUNSUPPORTED and the caller uses insv2v_gemm CONV3X3.  fp16 storage of V, U, M: 6.5e-4 of max|ref| vs fp32 conv2d (profiles/r06_winograd_proto.txt).
 * The two transforms are tested on their own, each against a float64 restatement (tests/winograd_ref.py) and bit for bit on inputs whose
 * intermediates are fp16 numbers: tests/test_winograd_stages_gpu.py (every launch regime of the input transform - several images per
 * workgroup with a partial last one, whole image at the LDS limit, bands with odd W, W = 128 -, strided x / x2 / residual / y / row_bias, what
 * must stay unwritten: rows [tiles, v_group_rows) of v, columns of y beyond Cout), tests/test_winograd_stages_cpu.py (the reference itself).
 */
typedef struct insv2v_winograd_in_desc {
    const void* x;
    const void* x2;      /* or NULL */
    const float* gn_ab;  /* or NULL: no normalisation */
    void* v;
    int64_t ldx, ldx2;
    int64_t v_group_rows;
    int32_t NB, H, W, C, C1;
    int32_t gn_images_per_sample;
    int32_t gn_silu;
    int32_t upsample;    /* 1: the convolution runs on the nearest-x2 upsampled image (Upsample3D, resnet.py:48-69): one tile per INPUT pixel,
                          *    9 matrices (groups g = ci*3 + cj over patch indices {0, 1, 3}^2; the others are identically zero), H, W need not be even */
} insv2v_winograd_in_desc;
int insv2v_winograd_input(const insv2v_winograd_in_desc* d, insv2v_stream_t stream);
typedef struct insv2v_winograd_out_desc {
    const void* m;
    const float* bias;      /* or NULL */
    const float* row_bias;  /* or NULL */
    const void* residual;   /* or NULL */
    void* y;
    int64_t m_group_rows;
    int64_t ldr, ldy, ld_rb;
    int32_t NB, H, W, Cout;   /* H, W: the INPUT image (upsample: y has NB * 2H * 2W rows) */
    int32_t rows_per_group;
    int32_t upsample;
} insv2v_winograd_out_desc;
int insv2v_winograd_output(const insv2v_winograd_out_desc* d, insv2v_stream_t stream);

/*
 * insv2v_ffn_fused: out = x + FeedForward_geglu(LayerNorm(x)) as ONE kernel, activations resident in registers, the hidden layer
 * never written (diffusers FeedForward behind norm3 / ff_norm: attention.py:259, motion_module.py:214,
 * i.e. LayerNorm -> Linear(C, 8C) -> h * gelu_erf(g) -> Linear(4C, C) -> + residual).  Supported: C = 320, hidden = 1280 (UNet level
 * 0); other widths return INSV2V_EUNSUPPORTED and the caller uses insv2v_gemm twice.
 * wstream: the layer's weights and biases (LayerNorm gamma / beta folded into the first projection) as ONE fp16 buffer of
 *   insv2v_ffn_stream_elems(C, hidden) elements in MFMA-fragment order - the order the kernel consumes it; layout documented in
 *   insv2v/fused.py (pack_ffn_stream), which is the reference packer.
 */
typedef struct insv2v_ffn_desc {
    const void* x;       /* [M, C] fp16, row stride ldx */
    void* out;           /* [M, C] fp16, row stride ldo (may not alias x) */
    const void* wstream; /* fp16 fragment stream */
    int64_t ldx, ldo;
    int32_t M, C, hidden;
    float eps;           /* LayerNorm eps */
    /* post != 0: the transformer module's trailing Linear (proj_out, attention.py:89 / motion_module.py:146) rides behind the feed-forward:
     *   out = Wp (x + FF(LN(x))) + bp + post_residual, Wp [C, C] appended to wstream (pack_ffn_stream(post=...)); the feed-forward result
     *   stays in registers.  post_residual: [M, C] fp16 (the module's input), row stride ld_post. */
    const void* post_residual;
    int64_t ld_post;
    int32_t post;
} insv2v_ffn_desc;
int insv2v_ffn_fused(const insv2v_ffn_desc* d, insv2v_stream_t stream);
int64_t insv2v_ffn_stream_elems(int32_t C, int32_t hidden, int32_t post);

/*
 * insv2v_rowlin: out = [LayerNorm](x) W^T + bias [+ residual] for the K = 320 / 640 Linear / 1x1-conv layers (UNet levels 0-1), activations
 * resident in registers (same machinery as insv2v_ffn_fused; csrc/rows_common.h): Transformer3DModel / TemporalTransformer3DModel
 * proj_in / proj_out (attention.py:64,89; motion_module.py:139,146), Attention.to_q / to_k / to_v / to_out
 * (attention.py:160-190, motion_module.py:289-331).  K must be 320 or 640 and N a multiple of 64, else INSV2V_EUNSUPPORTED (use insv2v_gemm).
 *   layernorm != 0: x is normalised per row in registers (no affine: gamma is folded into W and beta into the bias by the caller,
 *     exactly as for insv2v_gemm's folded LayerNorm) - no statistics pass and no row_stats;
 *   frame_bias != 0: the bias of row m is row (m / rows_per_frame) % frames of a per-frame table (the temporal positional encoding
 *     added after the norm, motion_module.py:277-278, pushed through W; frames <= 16), else a plain bias vector; both live in wstream;
 *   residual (optional): [M, N] fp16 added before the fp16 store.
 * wstream: insv2v_rowlin_stream_elems(N, K) fp16 elements in MFMA-fragment order (insv2v/fused.py pack_linear_stream).
 */
typedef struct insv2v_rowlin_desc {
    const void* x;        /* [M, K] fp16 */
    void* out;            /* [M, N] fp16 */
    const void* residual; /* [M, N] fp16 or NULL */
    const void* wstream;
    int64_t ldx, ldo, ldr;
    int32_t M, N, K;
    int32_t layernorm, frame_bias, rows_per_frame, frames;
    float eps;
    float* stats_out;     /* optional [M][2] fp32: (mean, rsqrt(var + stats_eps)) of the OUTPUT rows, i.e. finished LayerNorm statistics
                             for a following insv2v_gemm(row_stats=...) - a wave stores whole rows, so no partial sums are needed */
    float stats_eps;
    /* gn_ab != NULL (plain form only: no layernorm / frame_bias / residual): a preceding GroupNorm is applied to x on the fly,
     * x <- x * scale + shift with [samples][K][2] fp32 (scale, shift) pairs from insv2v_groupnorm(stats_only); row m belongs to sample
     * m / gn_rows.  Every gn_rows > 0 is accepted: each sample's rows are walked in 32-row wave blocks of its own (ceil(gn_rows / 32) per
     * sample; the overhang of the last one reads zeros and is never stored), which for gn_rows % 32 == 0 is the plain tiling of the M rows.
     * The transformer blocks' GroupNorm -> proj_in pair (attention.py:101-103, motion_module.py:136-139) without the normalised copy. */
    const float* gn_ab;
    int32_t gn_rows;
} insv2v_rowlin_desc;
int insv2v_rowlin(const insv2v_rowlin_desc* d, insv2v_stream_t stream);
int64_t insv2v_rowlin_stream_elems(int32_t N, int32_t K);
/* What insv2v_rowlin does with a descriptor, without doing it: the answer of the one planner (csrc/rows_plan.h) that insv2v_rowlin
 * consults before it launches.  A pure function of the descriptor's integers, the null and alignment bits of its pointers, the CU count
 * and the mask INSV2V_ROWLIN_TB2 (read once per process; bit `form` set: that K = 640 form may run two token blocks per wave); it touches
 * no GPU.  rowlin_kernel<ks, LN, FRAME, RES, gn, token_blocks> is the kernel: 2 x 8 forms with one token block per wave, 8 at K = 640 with
 * two (chosen where ceil(M / 256) >= 2 cus), and the GroupNorm-on-load form at both K.  A purely additive entry of ABI 15. */
typedef struct insv2v_rowlin_plan_t {
    int32_t rc;            /* 0, or what insv2v_rowlin returns without launching (INSV2V_EINVAL / INSV2V_EUNSUPPORTED) */
    int32_t ks;            /* 20 (K = 320) or 40 (K = 640) */
    int32_t form;          /* LN << 2 | FRAME << 1 | RES */
    int32_t gn;            /* the GroupNorm-on-load kernel */
    int32_t token_blocks;  /* TB: 1 or 2 */
    int32_t tile_rows;     /* 128 * TB */
    int32_t ntiles;        /* what the kernel loops over (gn: the 128-row tiles of the segmented schedule, four wave blocks each) */
    int32_t grid;          /* workgroups: min(ntiles, cus * wgs_per_cu) */
    int32_t rounds;        /* ceil(ntiles / grid): >= 2 means some workgroup takes a second tile */
    int32_t wgs_per_cu;    /* 2 at K = 320, 1 at K = 640 */
    int32_t lds_bytes;     /* dynamic LDS per workgroup */
    int32_t gn_units;      /* gn: 32-row wave blocks per sample = ceil(gn_rows / 32) */
} insv2v_rowlin_plan_t;
/* cus <= 0: this device's CU count (without a GPU there is none, and a problem that is otherwise accepted gets rc = INSV2V_EINVAL, as the
 * launch would).  Returns INSV2V_EINVAL for a NULL argument, else 0 with *out filled - also when out->rc says the problem is refused. */
int insv2v_rowlin_plan(const insv2v_rowlin_desc* d, int32_t cus, insv2v_rowlin_plan_t* out);

/*
 * insv2v_tattn_fused: one temporal self-attention sub-block of TemporalTransformerBlock (motion_module.py:206,270-336:
 * LayerNorm -> (+ positional encoding) -> to_q / to_k / to_v -> scaled-dot-product attention over the frames of every pixel ->
 * to_out -> + residual) as ONE register-resident launch.  Supported: C = 320, 8 heads, windows of 1 ... 32 frames (UNet level 0; the
 * stream layout holds 16 frame slots for 1 ... 16 frames and 32 for 17 ... 32, rows of padded slots are neither read nor written);
 * anything else returns INSV2V_EUNSUPPORTED and the caller uses insv2v_rowlin / insv2v_gemm + insv2v_attention.
 * x / out: token matrices [samples * frames * HW, C] fp16 with rows ordered (sample, frame, pixel).  wstream: insv2v_tattn_stream_elems()
 * fp16 elements from insv2v/fused.py pack_tattn_stream (q/k/v weights with the LayerNorm gamma folded in, the per-frame bias table
 * = positional-encoding rows pushed through the weights + W beta, the output projection and its bias).
 */
typedef struct insv2v_tattn_desc {
    const void* x;
    void* out;
    const void* wstream;
    int64_t ldx, ldo;
    int32_t samples, HW, C, heads, frames;
    float eps;   /* LayerNorm eps */
    float scale; /* softmax scale, head_dim^-0.5 */
} insv2v_tattn_desc;
int insv2v_tattn_fused(const insv2v_tattn_desc* d, insv2v_stream_t stream);
int64_t insv2v_tattn_stream_elems(int32_t C, int32_t heads, int32_t frames);
/* The same sub-block at C = 640 (8 heads x 80, 1 ... 32 frames) WITHOUT the output projection (ABI 8): out [rows, C] = the attention output
 * (LayerNorm -> q/k/v with the per-frame bias -> softmax over the frames -> P.V); to_out + residual follow as insv2v_rowlin.  q, k and v
 * never exist in memory.  Same descriptor; wstream: insv2v_tattn_attn_stream_elems(C, heads, frames) halfs (insv2v/fused.py
 * pack_tattn_qkv_stream). */
int insv2v_tattn_attn(const insv2v_tattn_desc* d, insv2v_stream_t stream);
int64_t insv2v_tattn_attn_stream_elems(int32_t C, int32_t heads, int32_t frames);

/*
 * Fused text cross-attention sub-block of BasicTransformerBlock (attention.py:249-257 = norm2 -> attn2 -> + residual, over diffusers
 * Attention: to_q of the tokens, to_k / to_v of the text context, to_out[0]) for C = 320, 8 heads x 40, 64 < ctx_len <= 96:
 *     out = x + Wo . softmax_keys( (LayerNorm(x) Wq^T + Wq beta) K_b^T * scale ) V_b + bo,   b = row / rows_per_sample
 * replaces insv2v_rowlin (q) + insv2v_attention + insv2v_rowlin (out-proj, residual).  x / out: [M, C] fp16 (row strides ldx / ldo;
 * out must not alias x), M a multiple of rows_per_sample.  Every rows_per_sample > 0 is accepted: each sample's rows are walked in 128-row
 * tiles of its own (ceil(rows_per_sample / 128) per sample; the overhang of the last one reads zeros and is never stored), which for
 * rows_per_sample % 128 == 0 is the plain tiling of the M rows.  The same holds for insv2v_xattn_attn.
 * wstream: insv2v_xattn_stream_elems(C, heads, 0) halfs - q projection (LayerNorm gamma folded in, bias = Wq beta) and output
 * projection as MFMA fragments; kvstream: [M / rows_per_sample] x insv2v_xattn_stream_elems(C, heads, 1) halfs - the text K / V of each
 * sample as fragments, masked per head and zero beyond ctx_len (insv2v/fused.py pack_xattn_stream / pack_xattn_kv).  The K / V of the
 * text are loop-invariant over the sampling loop, so the second stream is built once per prompt.
 */
typedef struct insv2v_xattn_desc {
    const void* x;
    void* out;
    const void* wstream;
    const void* kvstream;
    int64_t ldx, ldo;
    int32_t M, rows_per_sample, C, heads, ctx_len;
    float eps;   /* LayerNorm eps */
    float scale; /* softmax scale, head_dim^-0.5 */
    /* optional (insv2v_xattn_fused only): the out-projection of the preceding SELF-attention rides in front (attention.py:244-247):
     * x is then that attention's output, pre_residual [M, C] (row stride ld_pre) the tokens it is added to, and
     *     x1 = Wo1 . x + bo1 + pre_residual;   out = x1 + Wo . Attn(LayerNorm(x1) ...) + bo
     * with x1 never written to memory; wstream = insv2v_xattn_stream_elems(C, heads, 2) halfs (pack_xattn_stream(pre=...)). */
    const void* pre_residual;
    int64_t ld_pre;
} insv2v_xattn_desc;
int insv2v_xattn_fused(const insv2v_xattn_desc* d, insv2v_stream_t stream);
int64_t insv2v_xattn_stream_elems(int32_t C, int32_t heads, int32_t per_sample_kv);
/* The same sub-block at C = 640 (8 heads x 80) WITHOUT the output projection (ABI 8): out [M, C] = the attention output; to_out + residual
 * follow as insv2v_rowlin.  wstream: insv2v_xattn_attn_stream_elems(C, heads, 0) halfs (q projection only), kvstream: per sample
 * insv2v_xattn_attn_stream_elems(C, heads, 1) halfs (insv2v/fused.py pack_xattn_q_stream / pack_xattn640_kv). */
int insv2v_xattn_attn(const insv2v_xattn_desc* d, insv2v_stream_t stream);
int64_t insv2v_xattn_attn_stream_elems(int32_t C, int32_t heads, int32_t per_sample_kv);

/*
 * GroupNorm (+ optional SiLU) over channels-last data, both reduction domains of the path:
 *   5-D GroupNorm of ResnetBlock3D / conv_norm_out (resnet.py:177-178,188,194; unet.py:427-428):
 *     nsamples = b, rows_per_sample = f*h*w (statistics span all frames);
 *   per-frame GroupNorm of Transformer3DModel / TemporalTransformer3DModel and the VAE
 *     (attention.py:101; motion_module.py:136; vqvae/model.py:32-33): nsamples = b*f, rows = h*w.
 * Input may be a channel concat of two tensors (x: C1 channels, x2: C-C1 channels).
 * Pass 1 writes per-(sample,chunk,group) partial (sum, M2) to `partials`
 *   [nsamples, nchunks, G, 3] (count, mean, M2) fp32 placed after a [nsamples, G, 2] (mean, rstd) header in `partials`
 *   (total nsamples*G*(2+3*nchunks) floats); pass 2 merges them (Chan) into the header; pass 3 applies
 *   y = act((x-mean)*rstd*gamma+beta) into y [rows, C] fp16 (row stride ldy).
 */
typedef struct insv2v_groupnorm_desc {
    const void* x;
    const void* x2;
    void* y;
    const float* gamma;
    const float* beta;
    float* partials;
    int64_t ldx, ldx2, ldy;
    int32_t nsamples, rows_per_sample, C, C1, G;
    int32_t nchunks; /* chunks per sample used by pass 1 (>=1) */
    int32_t silu;
    float eps;
    /* stats_only != 0: passes 1-2 only; writes ab[nsamples][C][2] = (rstd*gamma, beta - mean*rstd*gamma) for a consumer
     * that applies y = act(x*scale + shift) itself (insv2v_gemm gn_ab); y may be NULL. */
    float* ab;
    int32_t stats_only;
} insv2v_groupnorm_desc;
int insv2v_groupnorm(const insv2v_groupnorm_desc* d, insv2v_stream_t stream);
/* What insv2v_groupnorm does with a descriptor, without doing it: the answer of the one planner (csrc/norm_plan.h) that insv2v_groupnorm
 * consults before it launches.  A pure function of the descriptor's integers, the null bits of its pointers and the two A/B switches
 * INSV2V_GN_FRAME / INSV2V_GN_FRAME_SPLIT (read once per process); it touches no GPU.  The planner enforces the whole-sample kernel's
 * reduction contract: the channel split is halved until G % cs == 0 and nt / (G / cs) is a power of two <= 64 (every split the dispatch
 * chooses by itself meets it; an override that does not is corrected, not run).  A purely additive entry of ABI 15: no existing struct or
 * entry changes. */
#define INSV2V_GN_PLAN_NONE 0       /* refused (rc != 0) */
#define INSV2V_GN_PLAN_THREE_PASS 1 /* gn_partial, gn_finalize and (without stats_only) gn_apply */
#define INSV2V_GN_PLAN_SMALL 2      /* gn_small<vw>: one workgroup per (sample, group) */
#define INSV2V_GN_PLAN_FRAME 3      /* gn_frame<nt>: one workgroup per (sample, channel part) */
typedef struct insv2v_groupnorm_plan_t {
    int32_t rc;             /* 0, or what insv2v_groupnorm returns without launching anything (INSV2V_EINVAL / INSV2V_EUNSUPPORTED) */
    int32_t family;         /* INSV2V_GN_PLAN_* */
    int32_t nt;             /* FRAME: threads per workgroup, 256 / 512 / 1024 */
    int32_t cs;             /* FRAME: channel parts per sample (grid y) */
    int32_t vw;             /* SMALL: halfs per load, 8 or 4 */
    int32_t p;              /* THREE_PASS: token lanes per workgroup, 1..16 */
    int32_t threads;        /* threads per workgroup of the kernel(s) that read x */
    int32_t nchunks;        /* THREE_PASS: the descriptor's nchunks clamped to rows_per_sample (the layout of `partials`); else 1 */
    int32_t rows_per_chunk; /* THREE_PASS: rows per chunk of pass 1 (trailing chunks may be empty); else rows_per_sample */
    int32_t apply_grid_x;   /* grid x of the launch that writes y: THREE_PASS gn_apply (0 with stats_only), SMALL G, FRAME nsamples */
    int32_t lds_bytes;      /* LDS per workgroup of the kernel that reads x */
} insv2v_groupnorm_plan_t;
/* Returns INSV2V_EINVAL for a NULL argument, else 0 with *out filled - also when out->rc says the problem is refused. */
int insv2v_groupnorm_plan(const insv2v_groupnorm_desc* d, insv2v_groupnorm_plan_t* out);

/*
 * LayerNorm over the channel axis of a token matrix [rows, C] (fp16 in/out, fp32 statistics,
 * eps inside the sqrt), optionally followed by the temporal positional-encoding add of
 * motion_module.py:236-242,277-278: y += pe[(row / rows_per_frame) % frames + pe_start, :]
 * (pe fp32 [max_len, C]).  Replaces nn.LayerNorm at attention.py:236,249,259 and
 * motion_module.py:206,214.
 */
typedef struct insv2v_layernorm_desc {
    const void* x;
    void* y;
    const float* gamma;
    const float* beta;
    const float* pe;
    int64_t ldx, ldy;
    int32_t rows, C;
    int32_t rows_per_frame, frames, pe_start;
    float eps;
} insv2v_layernorm_desc;
int insv2v_layernorm(const insv2v_layernorm_desc* d, insv2v_stream_t stream);
/* Per-token LayerNorm statistics only: stats[m] = (mean, rsqrt(var + eps)) of row m of x [rows, C] fp16.
 * Feeds the folded-LayerNorm epilogue of insv2v_gemm. */
int insv2v_layernorm_stats(const void* x, float* stats, int64_t ldx, int32_t rows, int32_t C, float eps,
                           insv2v_stream_t stream);

/*
 * Fused multi-head attention O = softmax(Q K^T * scale) V (flash style, MFMA for both
 * contractions, wave shuffles for the softmax reductions, fp32 online softmax).
 * Problem z in [0,batch): operand base = ptr + (z / *_inner) * *_outer + (z % *_inner) * *_step
 *   + head * head_dim; rows are *_rs apart.  This one addressing rule covers
 *   - spatial self-attention (attention.py:244 -> diffusers Attention, xformers in the reference):
 *     z = b*f, rows = h*w tokens;
 *   - text cross-attention (attention.py:251-256): K/V of sample z/f (kv_inner = f, kv_step = 0),
 *     seq_k = 77;
 *   - temporal self-attention over frames (motion_module.py:270-336, F.scaled_dot_product_attention
 *     in the reference): z = (b, pixel), rows = frames, row stride = h*w*ld.
 * head_dim is one of 16, 32, 40, 64, 80, 128, 160 or 512 (INSV2V_EUNSUPPORTED for another multiple of 8 up to 160, INSV2V_EINVAL for
 * anything else); seq_q, seq_k >= 1.
 * head_dim = 512 (the VAE's one-head mid AttnBlock, modules/vqvae/model.py:145-197): plain softmax only - causal != 0 or bias tables
 * return INSV2V_EUNSUPPORTED; any seq_q / seq_k / batch / heads.
 * Every head_dim: one problem's K and V rows have to lie within 2 GiB of its (problem, head) base, because the kernels load them
 * through one buffer descriptor with 32-bit byte offsets: (seq_k * max(k_rs, v_rs) + head_dim) * 2 > 0x7fffffff bytes returns
 * INSV2V_EUNSUPPORTED (the <= 16-row kernel loads only V that way: its rule is on v_rs alone).  The per-problem bases themselves are
 * 64-bit.  The row stride of temporal attention is h*w*ld, so a frame size alone can reach this.
 */
typedef struct insv2v_attention_desc {
    const void* q;
    const void* k;
    const void* v;
    void* o;
    int64_t q_rs, k_rs, v_rs, o_rs;
    int64_t q_outer, q_step, kv_outer, kv_step, o_outer, o_step;
    int32_t q_inner, kv_inner, o_inner;
    int32_t batch, heads, head_dim, seq_q, seq_k;
    float scale;
    int32_t causal; /* != 0: key j is visible to query i only if j <= i (CLIP text encoder, modules/openclip/modules.py:118) */
    /* ABI 8, optional (all three or none): fp16 tables [seq, ...] added to the rows of q / k / v as they are loaded - row i of the
     * sequence gets q_bias[i * bias_rs + head * head_dim + c].  This is the temporal positional encoding pushed through to_q / to_k /
     * to_v (motion_module.py:277-278 adds pe AFTER the norm, so it reaches all three): with the add here, the q/k/v projection in
     * front needs no per-frame row bias and may run on the persistent GEMM kernel.  Only the <= 16-row form (seq_q, seq_k <= 16, the
     * temporal attention over the frames) takes it; INSV2V_EUNSUPPORTED otherwise. */
    const void* q_bias;
    const void* k_bias;
    const void* v_bias;
    int64_t bias_rs;
} insv2v_attention_desc;
int insv2v_attention(const insv2v_attention_desc* d, insv2v_stream_t stream);
/* What insv2v_attention does with a descriptor, without doing it: the answer of the one planner (csrc/attn_plan.h) that insv2v_attention
 * consults before it launches.  A pure function of the descriptor's integers, the null and alignment bits of its pointers, the CU count
 * and the five A/B switches INSV2V_ATTN_SHORT / _FOLD / _SINGLE / _REP / _SHORT_WGS (read once per process); it touches no GPU.  A purely
 * additive entry of ABI 15: no existing struct or entry changes. */
#define INSV2V_ATTN_PLAN_NONE 0        /* refused (rc != 0) */
#define INSV2V_ATTN_PLAN_SHORT 1       /* attn_short_kernel<d>: <= 16 queries and keys, one workgroup per problem, one wave per head */
#define INSV2V_ATTN_PLAN_SHORT_BIAS 2  /* attn_short_kernel<d, true>: with the q / k / v bias tables, persistent over problems */
#define INSV2V_ATTN_PLAN_GENERIC 3     /* attn_kernel<d, nw, kvt, qb, fold>: double-buffered key tiles */
#define INSV2V_ATTN_PLAN_SINGLE 4      /* attn_kernel<160, 6, 96, 1, false, true>: the whole key sequence as one tile */
#define INSV2V_ATTN_PLAN_SINGLE_REP 5  /* ... one workgroup serving the kv_inner consecutive problems that share one K / V */
#define INSV2V_ATTN_PLAN_D512 6        /* attn_kernel<512, 4, 32, 1> */
typedef struct insv2v_attention_plan_t {
    int32_t rc;           /* 0, or what insv2v_attention returns without launching anything (INSV2V_EINVAL / INSV2V_EUNSUPPORTED) */
    int32_t family;       /* INSV2V_ATTN_PLAN_* */
    int32_t d;            /* template parameters: head dim, */
    int32_t nw;           /*   waves per workgroup (SHORT: = heads), */
    int32_t qb;           /*   16-row query blocks per wave, */
    int32_t kvt;          /*   keys per tile (SHORT: 16), */
    int32_t fold;         /*   the folded softmax (d = 40 / 80 with nw >= 4) */
    int32_t threads;      /* threads per workgroup */
    int32_t grid;         /* workgroups */
    int32_t lds_bytes;    /* dynamic LDS per workgroup */
    int32_t rows_per_wg;  /* query rows (over heads and problems) one workgroup serves: 16 nw qb; SINGLE_REP x kv_inner; SHORT 16 heads x the
                           * problems a persistent workgroup takes.  rows_per_wg * grid >= seq_q * heads * batch */
    int32_t ntiles;       /* key tiles per problem */
    int32_t ragged;       /* != 0: the last tile holds fewer than kvt keys (the masking path runs) */
} insv2v_attention_plan_t;
/* cus <= 0: this device's CU count (0 without a GPU: the persistent short kernel is then planned with one workgroup per problem).
 * Returns INSV2V_EINVAL for a NULL argument, else 0 with *out filled - also when out->rc says the problem is refused. */
int insv2v_attention_plan(const insv2v_attention_desc* d, int32_t cus, insv2v_attention_plan_t* out);

/*
 * Token + position embedding of the CLIP text encoder (transformers CLIPTextEmbeddings, called from
 * modules/openclip/modules.py:114-118): out[r, :] = tok[ids[r], :] + pos[r % L, :], fp16 tables, fp32 add, fp16 out.
 * ids: int64 device array of `rows` = n*L token ids, each in [0, vocab) (validated by the caller on the host).
 */
int insv2v_embed_tokens(const int64_t* ids, const void* tok, const void* pos, void* out, int32_t rows, int32_t L,
                        int32_t C, int32_t vocab, insv2v_stream_t stream);

/* Row softmax of an fp16 matrix [rows, cols] in place-capable form (VAE AttnBlock,
 * vqvae/model.py:186-188): y = softmax(x * scale) along cols. */
int insv2v_softmax_rows(const void* x, void* y, int64_t ldx, int64_t ldy, int32_t rows, int32_t cols,
                        float scale, insv2v_stream_t stream);
/* (ABI 13) The same over the first `valid` of `cols` columns (cols a multiple of 8): columns [valid, cols) are not read as values and are
 * written as exact zeros - the score matrix of a VAE AttnBlock whose h*w is not a multiple of 8, with its leading dimension padded to 8
 * so that P.V may contract over all `cols` columns (v^T's pad columns are zero too). */
int insv2v_softmax_rows_padded(const void* x, void* y, int64_t ldx, int64_t ldy, int32_t rows, int32_t cols, int32_t valid,
                               float scale, insv2v_stream_t stream);

/* Sinusoidal timestep features (diffusers Timesteps(dim, flip_sin_to_cos=True, shift) as used at
 * unet.py:95,358): out[b, :] = [cos(t*f_k), sin(t*f_k)] fp16, t read from device memory t[b] (fp32). */
int insv2v_timestep_embedding(const float* t, void* out, int32_t batch, int32_t dim, float shift,
                              insv2v_stream_t stream);

/*
 * (ABI 12) Second half of a 3x3 convolution (stride 1, zero padding 1) with <= 4 OUTPUT channels - the UNet's conv_out
 * (unet.py:432-434: InflatedConv3d(320, 4, 3, padding=1), resnet.py:14-21) at the stacked clip counts.  The first half is ONE
 * plain insv2v_gemm: y9[p, 4 t + c] = sum_ci x[p, ci] * W[c, ci, ky, kx], t = 3 ky + kx (fp32 out, >= 36 columns); this call adds the
 * nine shifted taps: out[p, c] = bias[c] + sum_t y9[p + (ky - 1) W + (kx - 1), 4 t + c] over the taps inside the image (fp32,
 * c < cout <= 4).  ld9 / ldo in fp32 elements, ld9 a multiple of 4, y9 16-byte aligned.  NB images of H x W pixels, row-major.
 */
int insv2v_tap_gather(const float* y9, int64_t ld9, const float* bias, float* out, int64_t ldo, int32_t NB, int32_t H, int32_t W,
                      int32_t cout, insv2v_stream_t stream);

/*
 * Build the 3-way classifier-free-guidance UNet input of inference.py:183-189 in channels-last
 * fp16: out[3, F, h, w, ldo] with channels [latent(4) | 0 or img_cond(4) | zero pad], from
 * latent/img_cond fp32 in the reference layout [F, 4, h, w].  Also writes `timestep` to t_out[0..2].
 * nbranch = 3 (text/video CFG) or 1 (CFG off: latent | img_cond).
 */
int insv2v_build_unet_input(const float* latent, const float* img_cond, void* out, float* t_out,
                            float timestep, int32_t nbranch, int32_t F, int32_t h, int32_t w, int32_t ldo,
                            int64_t branch_rows, int32_t t_stride, insv2v_stream_t stream);
/* (ABI 10) branch_rows = rows of `out` between consecutive branches (0 = F*h*w: the clip's branches back to back), t_stride = entries
 * of t_out between them (0 = 1): a stack of n clips laid out BRANCH-major ([branch][clip] samples, so that the two branches that share
 * their UNet input - (no text, video) and (text, video) - form one contiguous range) passes n*F*h*w and n.  The same stride, in fp32
 * elements, is insv2v_step_desc.branch_stride / the branch_stride argument of insv2v_cfg_stats for the UNet output. */

/*
 * Fused CFG combine + long-video noise correction + scheduler step (inference.py:198-210,
 * :270-277; diffusers DDIMScheduler.step / DDPMScheduler.step):
 *   eps = n1 + img_cfg*(n2-n1) + text_cfg*(n3-n2)            (nbranch==3; else eps = n1)
 *   [guidance rescale, inference.py:13-24, when rescale > 0: needs eps_stats from insv2v_cfg_stats]
 *   [correction, when R > 0: d_r = (latent_r - sqrt_a*latent_ref_r)/sqrt_1ma - eps_r for r<R;
 *      eps_r += d_r; eps_q += mean_r d_r for q>=R  (flow==NULL)  or the flow-warped masked average
 *      of inference.py:374-386 (delta_q supplied by insv2v_flow_correction)]
 *   x0 = (latent - sqrt_1ma*eps)/sqrt_a;  prev = c_x0*x0 + c_eps*eps + c_xt*latent + c_noise*noise
 * eps_in: fp32 [nbranch, F, h, w, 4] channels-last (UNet conv_out output); latent, latent_out,
 * pred_x0, eps_out: fp32 [F,4,h,w] (reference layout).  eps_out/pred_x0/noise may be NULL.
 */
typedef struct insv2v_step_desc {
    const float* eps_in;
    const float* latent;
    const float* latent_ref; /* [R,4,h,w] or NULL */
    const float* delta_q;    /* [F-R,4,h,w] precomputed flow correction for query frames or NULL */
    const float* noise;      /* DDPM variance noise [F,4,h,w] or NULL */
    const float* rescale_stats; /* device [2]: std_text, std_cfg or NULL */
    float* latent_out;
    float* pred_x0;
    float* eps_out;
    int32_t nbranch, F, h, w, R;
    int32_t correct; /* 0 none, 1 mean over refs, 2 use delta_q */
    float text_cfg, img_cfg;
    float sqrt_a, sqrt_1ma;       /* sqrt(alpha_bar_t), sqrt(1-alpha_bar_t) */
    float c_x0, c_eps, c_xt, c_noise;
    float guidance_rescale;
    int64_t branch_stride; /* fp32 elements of eps_in between consecutive branches; 0 = F*h*w*4 */
    /* (ABI 14) noise == NULL, noise_on != 0 and c_noise != 0: the variance noise [F,4,h,w] is generated inside the kernel, element
     * (flat index) i of it = element i of the normal stream (noise_seed, noise_stream) of the section "seeded noise" - bit-identical
     * to insv2v_randn into a tensor passed as `noise`, without that tensor.  noise_on != 0 with a non-NULL noise: INSV2V_EINVAL. */
    int64_t noise_seed, noise_stream;
    int32_t noise_on;
} insv2v_step_desc;
int insv2v_cfg_step(const insv2v_step_desc* d, insv2v_stream_t stream);
/*
 * Multistep form of insv2v_cfg_step (DPM-Solver++ 2M in its data-prediction form, ODE and SDE): the same kernel body with one more
 * term, a coefficient times the PREVIOUS step's x0 prediction:
 *   prev = c_x0*x0 + c_eps*eps + c_xt*latent + c_hist*x0_hist + c_noise*noise
 * Everything in front of that line - CFG combine, guidance rescale, correction modes, nbranch, branch_stride, eps_out / pred_x0, the
 * seeded in-kernel noise - is insv2v_cfg_step's, and with x0_hist == NULL the call runs insv2v_cfg_step's own kernel (bit-identical results).  The descriptor holds
 * the fields of insv2v_step_desc in their order, then:
 *   x0_hist  fp32 [F,4,h,w] (reference layout) or NULL: the pred_x0 output of the previous executed step.  It is read while the
 *            outputs are written: a range that overlaps latent_out, pred_x0 or eps_out returns INSV2V_EINVAL.
 *   c_hist   its coefficient; c_hist != 0 with x0_hist == NULL returns INSV2V_EINVAL.
 * An addition to ABI 14: insv2v_step_desc and insv2v_cfg_step are unchanged.
 */
typedef struct insv2v_mstep_desc {
    const float* eps_in;
    const float* latent;
    const float* latent_ref;
    const float* delta_q;
    const float* noise;
    const float* rescale_stats;
    float* latent_out;
    float* pred_x0;
    float* eps_out;
    int32_t nbranch, F, h, w, R;
    int32_t correct;
    float text_cfg, img_cfg;
    float sqrt_a, sqrt_1ma;
    float c_x0, c_eps, c_xt, c_noise;
    float guidance_rescale;
    int64_t branch_stride;
    int64_t noise_seed, noise_stream;
    int32_t noise_on;
    const float* x0_hist;
    float c_hist;
} insv2v_mstep_desc;
int insv2v_cfg_step_ms(const insv2v_mstep_desc* d, insv2v_stream_t stream);
/*
 * Masked form of insv2v_cfg_step_ms (localized and partial edits): the same kernel body with one more pass behind the scheduler update,
 * which holds the region outside the mask at the source video's latent re-noised to the level the step's output lives at:
 *   known      = k_src*src + k_noise*known_noise            (k_src = sqrt(alpha_bar_prev), k_noise = sqrt(1 - alpha_bar_prev))
 *   latent_out = mask*prev + (1 - mask)*known               (mask 1 = edit, 0 = keep; broadcast over the 4 channels)
 * pred_x0 and eps_out stay the model's own (unblended), so the multistep history keeps reading the model's prediction.  Everything in
 * front of the blend - CFG combine, guidance rescale, correction modes, nbranch, branch_stride, injected / seeded variance noise, the
 * history term - is insv2v_cfg_step_ms's.  With mask == NULL the call IS insv2v_cfg_step_ms (the same kernels: bit-identical results).
 * The descriptor holds the fields of insv2v_mstep_desc in their order, then:
 *   mask         fp32 [F,h,w] in [0,1] or NULL
 *   src          fp32 [F,4,h,w]: the scaled source latent (what the VAE encoder returns times the scale factor)
 *   known_noise  fp32 [F,4,h,w]: the fixed noise the source is re-noised with (the window's initial noise)
 *   k_src, k_noise
 * INSV2V_EINVAL: a mask without src or known_noise; a mask with latent_out == NULL; F, h or w <= 0; mask, src, known_noise or x0_hist
 * overlapping the range of latent_out, pred_x0 or eps_out (they are read while those are written).
 * An addition to ABI 14: the existing descriptors and entries are unchanged.
 */
typedef struct insv2v_maskstep_desc {
    const float* eps_in;
    const float* latent;
    const float* latent_ref;
    const float* delta_q;
    const float* noise;
    const float* rescale_stats;
    float* latent_out;
    float* pred_x0;
    float* eps_out;
    int32_t nbranch, F, h, w, R;
    int32_t correct;
    float text_cfg, img_cfg;
    float sqrt_a, sqrt_1ma;
    float c_x0, c_eps, c_xt, c_noise;
    float guidance_rescale;
    int64_t branch_stride;
    int64_t noise_seed, noise_stream;
    int32_t noise_on;
    const float* x0_hist;
    float c_hist;
    const float* mask;
    const float* src;
    const float* known_noise;
    float k_src, k_noise;
} insv2v_maskstep_desc;
int insv2v_cfg_step_mask(const insv2v_maskstep_desc* d, insv2v_stream_t stream);
/*
 * Released form of insv2v_cfg_step_mask (per-pixel edit strength; tests/strength_map_ref.py is the definition):
 * every latent cell carries the index of the step that releases it to the model, and until then it is held like a cell outside the mask:
 *   m_eff      = release[f,y,x] <= step ? m : 0             (m = mask[f,y,x], or 1 with mask == NULL)
 *   latent_out = m_eff*prev + (1 - m_eff)*known             (known as for insv2v_cfg_step_mask)
 * `step` is the GLOBAL index of the step in the scheduler's timesteps (start_time + i of a partial edit), the index `release` was built
 * against (insv2v_strength_release).  The gate is the only new arithmetic: the blend expression behind it is the mask form's, and pred_x0
 * and eps_out stay the model's own.  With release == NULL the call IS insv2v_cfg_step_mask (the same kernels: bit-identical results).
 * The descriptor holds the fields of insv2v_maskstep_desc in their order, then:
 *   release      int32 [F,h,w] or NULL
 *   step         >= 0
 * INSV2V_EINVAL (before any launch): a release map without src, known_noise or latent_out; step < 0; F, h or w <= 0; release, mask, src,
 * known_noise or x0_hist overlapping the range of latent_out, pred_x0 or eps_out.
 * An addition to ABI 15: the existing descriptors, entries and kernels are unchanged.
 */
typedef struct insv2v_relstep_desc {
    const float* eps_in;
    const float* latent;
    const float* latent_ref;
    const float* delta_q;
    const float* noise;
    const float* rescale_stats;
    float* latent_out;
    float* pred_x0;
    float* eps_out;
    int32_t nbranch, F, h, w, R;
    int32_t correct;
    float text_cfg, img_cfg;
    float sqrt_a, sqrt_1ma;
    float c_x0, c_eps, c_xt, c_noise;
    float guidance_rescale;
    int64_t branch_stride;
    int64_t noise_seed, noise_stream;
    int32_t noise_on;
    const float* x0_hist;
    float c_hist;
    const float* mask;
    const float* src;
    const float* known_noise;
    float k_src, k_noise;
    const int32_t* release;
    int32_t step;
} insv2v_relstep_desc;
int insv2v_cfg_step_release(const insv2v_relstep_desc* d, insv2v_stream_t stream);
/*
 * Strength image -> release map and pixel gate, one launch, no atomics, no read-back:
 *   s_c     = the cell value insv2v_mask_to_latent(smap, mode) gives, bit for bit (the same device function)
 *   n_exec  = 0 if s_c <= 0 or NaN, else min(steps, max(1, floor((double)s_c * steps + 0.5)))   (formed in double: exact for steps <= 2^20)
 *   release [N,H/8,W/8] int32 = steps - n_exec            (in [0, steps]; steps = the cell is never released)
 *   gate    [N,H,W] fp32      = 0 where smap <= 0 or NaN, elsewhere mask_img (or 1 with mask_img == NULL); not written when gate == NULL
 * INSV2V_EINVAL: H or W not a positive multiple of 8; N <= 0; steps outside [1, 2^20]; mode not 0 or 1; NULL smap or release; gate
 * overlapping smap or mask_img.
 */
int insv2v_strength_release(const float* smap, const float* mask_img, int32_t* release, float* gate, int32_t N, int32_t H, int32_t W,
                            int32_t mode, int32_t steps, insv2v_stream_t stream);
/* Image-resolution mask fp32 [N,H,W] -> latent resolution [N,H/8,W/8]: per 8x8 cell its mean (mode 0; a pairwise sum, so a mask in
 * [0,1] is within 6 * 2^-24 of the exact mean) or its maximum (mode 1).  H and W must be positive multiples of 8 (any such size);
 * everything else returns INSV2V_EINVAL. */
int insv2v_mask_to_latent(const float* mask, float* out, int32_t N, int32_t H, int32_t W, int32_t mode, insv2v_stream_t stream);
/* out = clip(mask*edited + (1 - mask)*original, -1, 1) on fp32 [N,3,H,W] frames, mask fp32 [N,H,W] at image resolution (broadcast over
 * the channels).  out may alias edited (each element is read before it is written, by the same thread). */
int insv2v_composite(const float* edited, const float* original, const float* mask, float* out, int32_t N, int32_t H, int32_t W,
                     insv2v_stream_t stream);
/* out = ka*z + kb*noise over n fp32 elements (the source latent re-noised to a step's level; out may alias z or noise). */
int insv2v_add_noise(const float* z, const float* noise, float* out, int64_t n, float ka, float kb, insv2v_stream_t stream);
/* std over all elements of n1 (branch 1) and of the CFG-combined eps -> stats[0..1] (inference.py:18-19). */
int insv2v_cfg_stats(const float* eps_in, float* stats, int32_t F, int32_t h, int32_t w, float text_cfg,
                     float img_cfg, int64_t branch_stride, insv2v_stream_t stream);

/* warp_image of misc_utils/flow_utils.py:25-57: bilinear grid_sample(align_corners=True, zero
 * padding) of image [N,C,H,W] fp32 at (x+flow_x, y+flow_y); flow [N,2,H,W] fp32. */
int insv2v_warp_image(const float* image, const float* flow, float* out, int32_t N, int32_t C, int32_t H,
                      int32_t W, insv2v_stream_t stream);
/* resize_flow of misc_utils/flow_utils.py:59-86: scale (u,v) by (W/w, H/h) then bilinear resize
 * (align_corners=False) [N,2,h,w] -> [N,2,H,W]. */
int insv2v_resize_flow(const float* flow, float* out, int32_t N, int32_t h, int32_t w, int32_t H, int32_t W,
                       insv2v_stream_t stream);
/*
 * Flow-warped noise correction for the query frames (inference.py:296-301, :374-386):
 * eps_cfg fp32 [F,4,h,w] is the CFG-combined noise; delta_r = (latent_r - sqrt_a*ref_r)/sqrt_1ma - eps_r;
 * for each query q: out_q = sum_r warp(delta_r, flow_qr) / sum_r warp(1, flow_qr) where the mask
 * sum > 0.5, else 0.  flows: fp32 [F-R, R, 2, h, w] already at latent resolution.
 */
int insv2v_flow_correction(const float* eps_cfg, const float* latent, const float* latent_ref,
                           const float* flows, float* delta_q, int32_t F, int32_t R, int32_t h, int32_t w,
                           float sqrt_a, float sqrt_1ma, insv2v_stream_t stream);

/* Layout conversions at the VAE boundary (instruct_p2p_video.py:57-79):
 * frames fp32 [N,C,H,W] -> fp16 [N,H,W,ldo] (zero channel pad) and back (with optional scale). */
int insv2v_nchw_to_nhwc_f16(const float* x, void* y, int32_t N, int32_t C, int32_t H, int32_t W, int32_t ldo,
                            float scale, insv2v_stream_t stream);
int insv2v_nhwc_to_nchw_f32(const void* x, int32_t x_is_fp32, float* y, int32_t N, int32_t C, int32_t H,
                            int32_t W, int32_t ldx, float scale, insv2v_stream_t stream);
/* Diagonal-Gaussian posterior sample of kl_autoencoder/autoencoder.py:10-23, times `scale`:
 * moments fp32 [N,H,W,8] channels-last (mean|logvar) + noise fp32 [N,4,H,W] -> z fp32 [N,4,H,W]. */
int insv2v_posterior_sample(const float* moments, const float* noise, float* z, int32_t N, int32_t H,
                            int32_t W, int32_t ldm, float scale, insv2v_stream_t stream);
/* (ABI 14) The same with the noise generated inside the kernel: element i of the [N,4,H,W] sample takes element offset + i of the normal
 * stream (seed, stream) of the section "seeded noise".  offset = flat index of this call's first frame inside the video's [T,4,H,W], so
 * a video encoded in several calls gets the sample of one call.  Bit-identical to insv2v_randn + insv2v_posterior_sample. */
int insv2v_posterior_sample_seeded(const float* moments, float* z, int32_t N, int32_t H, int32_t W, int32_t ldm, float scale,
                                   int64_t seed, int64_t stream, int64_t offset, insv2v_stream_t hip_stream);

/*
 * ---- seeded noise (ABI 14) -----------------------------------------------------------------------------------------------------------
 * Every random draw of the sampling path (VAE posterior noise, initial latents, DDPM variance noise) can come from a counter-based
 * generator, so that a value is a pure function of (seed, stream id, element index) - independent of call order, of how units are
 * stacked or split, and of the number of GPUs.  The definition below is a PUBLIC CONTRACT: it does not change between versions (a
 * checkpointed experiment must replay), and tests/philox_ref.py restates it in numpy.
 *
 *   generator   Philox4x32-10 (Salmon et al., SC'11; the Random123 known answers hold): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key
 *               increments 0x9E3779B9 / 0xBB67AE85, ten rounds.
 *   key         (seed & 0xffffffff, seed >> 32); seed is an int64_t taken as its two's-complement bits.
 *   counter     (block & 0xffffffff, block >> 32, stream & 0xffffffff, stream >> 32), block = element index >> 2.
 *   element i   output word i & 3 of block i >> 2: any sub-range can be generated on its own and is bit-identical to the same range
 *               of a longer draw.
 *   uniform     u = ((word >> 8) + 0.5) * 2^-24, strictly inside (0, 1).
 *   normal      Box-Muller per pair of words of a block: z0 = r0 cos(2 pi u1), z1 = r0 sin(2 pi u1), r0 = sqrt(-2 ln u0); z2, z3 likewise
 *               from u2, u3.  |z| <= 5.89.  The kernels evaluate this in fp32 from exact images of the words (csrc/rng.h); the error
 *               against a float64 evaluation is recorded in DESIGN.md.
 *   stream id   what the host packs per purpose (insv2v/rng.py stream_id(kind, unit, window, step)); the kernels take any int64_t:
 *                 bits 52-53 kind (0 ENC, 1 INIT, 2 STEP, 3 MASK) | bits 28-51 unit (< 2^24) | bits 16-27 window (< 2^12) | bits 0-15 step (< 2^16)
 *               ENC : element index over the whole video's posterior noise [T,4,h,w] (window = step = 0);
 *               INIT: element index over the NEW frames [n,4,h,w] of window k (the overlap re-uses the previous window's initial noise);
 *               STEP: element index over the clip's [F,4,h,w] at window k, sampling step i;
 *               MASK: element index over the chunk's [F,4,h,w] of the mask estimate (section "a mask estimated from the prompt"):
 *                     window = index of the chunk, step = index of the draw.
 *
 * insv2v_randn writes elements [offset, offset + n) of the stream (seed, stream) to out: fp32 normals, or with raw = 1 the 32-bit words'
 * bit patterns.  n and offset are 64-bit (offset + n may cross a multiple of 2^34, where the block index carries into its high word);
 * out needs 4-byte alignment only.  n < 0, offset < 0, an index range beyond int64 or raw outside {0, 1}: INSV2V_EINVAL.
 */
int insv2v_randn(float* out, int64_t n, int64_t seed, int64_t stream, int64_t offset, int32_t raw, insv2v_stream_t hip_stream);

/*
 * ---- optical-flow estimator (ABI 9) --------------------------------------------------------------------------------------------------
 * The kernels behind RAFTFlow (misc_utils/flow_utils.py:134-189; built at pl_trainer/inference/inference.py:294, called per query
 * frame at :303-311).  The network itself is third-party (torchvision raft_large, not under the reference tree): every convolution of it
 * is insv2v_im2col + insv2v_gemm (LINEAR; bias and ReLU / sigmoid / tanh in the epilogue), the rest are the entries below.
 * Activations are channels-last fp16 token matrices [n*h*w, C], correspondences and flows fp32 [n, 2, h, w] as in the reference.
 */
typedef struct insv2v_im2col_desc {
    const void* x;   /* fp16 [N*IH*IW, C1 of ldx]: input channels [0, C1) */
    const void* x2;  /* optional second source: channels [C1, C) (row stride ldx2) - torch.cat along channels, never materialised */
    void* out;       /* fp16 [N*OH*OW, ldo]; column (ky * KW + kx) * C + c; zero outside the image */
    int64_t ldx, ldx2, ldo;
    int32_t N, IH, IW, C, C1, KH, KW, stride_h, stride_w, pad_h, pad_w, OH, OW;
} insv2v_im2col_desc;
/* F.conv2d's input gather for kernels the implicit-GEMM path does not cover (7x7 stride 2, 1x5, 5x1, 1x1 stride 2, channel counts
 * that are no multiple of 64): C, C1 multiples of 8.  OH / OW must equal floor((I + 2 pad - K) / stride) + 1. */
int insv2v_im2col(const insv2v_im2col_desc* d, insv2v_stream_t stream);
/* nn.InstanceNorm2d (affine=False, biased variance) + optional ReLU over [N, HW, C] fp16 (torchvision's feature encoder);
 * y != x; partials = fp32 scratch of N * nchunks * C * 2 floats; deterministic (no atomics), shifted sums. */
int insv2v_instance_norm(const void* x, void* y, float* partials, int32_t N, int32_t HW, int32_t C, int64_t ldx, int64_t ldy,
                         int32_t nchunks, float eps, int32_t relu, insv2v_stream_t stream);
#define INSV2V_EW_RELU 1     /* out = relu(a) */
#define INSV2V_EW_ADD_RELU 2 /* out = relu(a + b): ResidualBlock */
#define INSV2V_EW_TANH 3     /* out = tanh(a): initial hidden state */
#define INSV2V_EW_GRU_RH 4   /* out = a * b: ConvGRU r * h (a already sigmoid-ed) */
#define INSV2V_EW_GRU_OUT 5  /* out = (1 - c) * b + c * a: ConvGRU h' = (1 - z) h + z q */
int insv2v_ew(int32_t op, const void* a, const void* b, const void* c, void* out, int64_t rows, int32_t C, int64_t lda, int64_t ldb,
              int64_t ldc, int64_t ldo, insv2v_stream_t stream);
/* F.avg_pool2d(kernel 2, stride 2) over the last two dims of fp32 [n, h, w]: one level of CorrBlock.build_pyramid */
int insv2v_avgpool2x2(const float* x, float* y, int64_t n, int32_t h, int32_t w, insv2v_stream_t stream);
typedef struct insv2v_corr_lookup_desc {
    const float* pyr0;   /* level l: fp32 [B*h*w, h >> l, w >> l] (the all-pairs correlation and its pooled copies) */
    const float* pyr1;
    const float* pyr2;
    const float* pyr3;
    const float* coords; /* fp32 [B, 2, h, w]: current correspondences (x, y) */
    void* out;           /* fp16 [B*h*w, ldo]: levels * (2 radius + 1)^2 look-ups per pixel, remaining columns zero */
    int64_t ldo;
    int32_t B, h, w, levels, radius;
} insv2v_corr_lookup_desc;
/* CorrBlock.index_pyramid: bilinear (align_corners=True, zero padding) samples at coords / 2^l + (d_i, d_j), d in [-radius, radius];
 * channel l * side^2 + i * side + j, the FIRST offset applied to x (torchvision's delta order). */
int insv2v_corr_lookup(const insv2v_corr_lookup_desc* d, insv2v_stream_t stream);
/* coords1 += delta (fp32 rows [B*h*w, ldd], columns 0 / 1; NULL = no update), then rows[pix][0..1] = coords1 - pixel grid as fp16
 * (columns 2 .. ncols-1 zero; rows may be NULL): the flow fed to the motion encoder and appended to its output */
int insv2v_raft_flow_rows(float* coords1, const float* delta, int64_t ldd, void* rows, int64_t ldf, int32_t ncols, int32_t B, int32_t h,
                          int32_t w, insv2v_stream_t stream);
/* upsample_flow: convex combination of the 3x3 neighbourhood of 8 * (coords1 - grid) with softmax weights from the mask predictor's
 * 576 logits per pixel (fp16 rows, k * 64 + i * 8 + j) -> fp32 [B, 2, 8h, 8w] */
int insv2v_convex_upsample(const float* coords1, const void* mask, int64_t ldm, float* out, int32_t B, int32_t h, int32_t w,
                           insv2v_stream_t stream);

/*
 * ---- scoring an edit with CLIP (additions to ABI 15: no existing struct or entry changes) -----------------------------------------------
 * The kernels behind ClipSimilarity (misc_utils/clip_similarity.py:10-47) that are not insv2v_gemm / insv2v_layernorm / insv2v_attention.
 */
typedef struct insv2v_clip_preprocess_desc {
    const void* x;        /* frames [n, 3, H, W], fp16 or fp32 (x_fp32), element strides below: any view of a larger tensor */
    void* out;            /* fp16 [n * (S/P)^2, ld]: patch rows in (frame, patch row, patch column) order, column c*P*P + py*P + px - the
                           * flattened patch_embedding.weight [C, 3, P, P] order; columns [3*P*P, ld) are written as exact zeros */
    int64_t stride_n, stride_c, stride_h, stride_w;
    int64_t ld;
    int32_t n, H, W, S, P, x_fp32;
    float in_scale, in_shift;   /* pixel = in_scale * x + in_shift maps the frames to [0, 1] (0.5, 0.5 for frames in [-1, 1]) */
    float mean[3], std[3];      /* per channel: (pixel - mean) / std */
} insv2v_clip_preprocess_desc;
/* encode_image's pixel front end (:29-31) in one pass, no intermediate image: F.interpolate(size = (S, S), mode = "bicubic",
 * align_corners = False) - source coordinate (dst + 0.5) * in / out - 0.5 NOT clamped, cubic convolution with A = -0.75, the 4 x 4 tap
 * indices clamped to the border, no antialias, the overshoot of the cubic NOT clamped - then (pixel - mean_c) / std_c; fp32 arithmetic,
 * one fp16 rounding of the stored value.  S x S is square whatever the frame's aspect, as in the reference.
 * INSV2V_EINVAL: S % P != 0, ld < 3*P*P, n / H / W / S / P <= 0, a std that is not positive, x or out NULL. */
int insv2v_clip_preprocess(const insv2v_clip_preprocess_desc* d, insv2v_stream_t stream);
/* The metrics of frame i from the towers' features: img0 / img1 [n, D] (row strides ld0 / ld1 elements), txt0 / txt1 [D] for every frame
 * (ldt = 0) or [n, D] (row stride ldt); all four fp16, or all four fp32 (fp32 != 0).  Every operand is L2-normalised first (:25, :33: no
 * eps), then out[i] (fp32 [n, 5]) =
 *   sim_0 = cos(img0, txt0), sim_1 = cos(img1, txt1), sim_direction = cos(img1 - img0, txt1 - txt0), sim_image = cos(img0, img1),
 *   consistency = cos(img1[i], img1[i + 1]) with the last frame's entry exact 0,
 * where cos(x, y) = sum(x / max(|x|, eps) * y / max(|y|, eps)) is F.cosine_similarity (each norm clamped on its own; eps 1e-8 there).
 * fp32 sums in a fixed order: two calls give the same bits.  INSV2V_EINVAL: n or D <= 0, a row stride below D (ldt: other than 0),
 * eps <= 0, a NULL pointer. */
int insv2v_clip_scores(const void* img0, const void* img1, const void* txt0, const void* txt1, int32_t fp32, int64_t ld0, int64_t ld1,
                       int64_t ldt, int32_t n, int32_t D, float eps, float* out, insv2v_stream_t stream);
/* out[i] (fp32, row stride ldo) = x[i] / |x[i]| for the n rows of x [n, D] (fp16, or fp32 with fp32 != 0; row stride ldx): the last line
 * of encode_image / encode_text (:25, :33; no eps, as there).  out may be x when x is fp32.  INSV2V_EINVAL: n or D <= 0, a row stride
 * below D, a NULL pointer. */
int insv2v_l2_normalize(const void* x, int32_t fp32, int64_t ldx, float* out, int64_t ldo, int32_t n, int32_t D, insv2v_stream_t stream);

/*
 * ---- a mask estimated from the prompt (additions to ABI 15: no existing struct or entry changes) --------------------------------------
 * Branches 1 and 2 of the 3-way CFG stack see the same latent and the same video condition and differ only in the text, so
 * |eps3 - eps2| says where the instruction acts.  Averaged over n noised copies of the source latent, normalised by the video's mean,
 * smoothed, thresholded and dilated it is the mask of a localized edit (DiffEdit's recipe; csrc/automask.hip, DESIGN.md section 18,
 * tests/automask_ref.py restates the definition in float64).
 */
/* insv2v_build_unet_input for nbranch = 3 (same out / t_out layout, branch_rows, t_stride) whose latent channels are
 * ka * latent + kb * noise: noise = the tensor `noise` [F,4,h,w] (seeded = 0), or element (flat index of [F,4,h,w]) i of the normal
 * stream (seed, noise_stream) of the section "seeded noise" (seeded = 1, noise = NULL).  The fp16 values are bit-identical to
 * insv2v_add_noise (after insv2v_randn for the seeded form) followed by insv2v_build_unet_input.  INSV2V_EINVAL: a NULL latent /
 * img_cond / out, F, h or w <= 0, ldo < 8, both a tensor and seeded = 1 or neither, branch_rows below F*h*w (other than 0). */
int insv2v_build_unet_input_noised(const float* latent, const float* img_cond, const float* noise, void* out, float* t_out,
                                   float timestep, float ka, float kb, int64_t seed, int64_t noise_stream, int32_t seeded,
                                   int32_t F, int32_t h, int32_t w, int32_t ldo, int64_t branch_rows, int32_t t_stride,
                                   insv2v_stream_t stream);
/* acc[F,h,w] (accumulate = 0: =, 1: +=) scale * sum over the 4 channels of |eps[2 bs + 4 pix + c] - eps[bs + 4 pix + c]|: eps is the
 * UNet's channels-last fp32 output, bs = branch_stride fp32 elements between the branches (0 = 4*F*h*w) exactly as
 * insv2v_step_desc.branch_stride; branch 0 and everything outside the two [F*h*w, 4] blocks is never read.  eps must be 16-byte
 * aligned and bs a multiple of 4 (one 16-byte load per pixel and branch).  Order: s = (|d0| + |d1|) + (|d2| + |d3|), then
 * acc = fma(scale, s, acc), or scale * s when accumulate = 0 (no memset is needed in front of the first draw). */
int insv2v_eps_absdiff_accum(const float* eps, float* acc, int32_t F, int32_t h, int32_t w, int64_t branch_stride, float scale,
                             int32_t accumulate, insv2v_stream_t stream);
/* Bytes of workspace insv2v_automask_finish needs for a [T,h,w] map (the partial sums of its mean); INSV2V_EINVAL for a size <= 0. */
int64_t insv2v_automask_workspace_bytes(int32_t T, int32_t h, int32_t w);
/* raw fp32 [T,h,w] (>= 0) -> soft [T,h,w], mask_latent [T,h,w] (0 / 1) and mask [T,8h,8w] (every cell replicated 8 x 8, so
 * insv2v_mask_to_latent returns mask_latent in both modes):
 *   mean = mean(raw) over the whole map, a fixed-order fp32 reduction without atomics (two runs give the same bits);
 *   soft0 = min(raw, clamp_ratio * mean) / (clamp_ratio * mean), 0 everywhere when mean == 0 (no division);
 *   soft = soft0, or with smooth = 1 its temporal binomial [1,2,1]/4 over the T frames followed by the spatial 3 x 3 binomial
 *          [1,2,1] x [1,2,1] / 16, edges replicated in both (T = 1: spatial only);
 *   bin = soft > threshold (strict); mask_latent = max of bin over the (2 dilate + 1)^2 spatial square, zeros outside the frame.
 * Nothing is allocated: the caller passes workspace (4-byte aligned) of at least insv2v_automask_workspace_bytes(T,h,w) bytes.
 * INSV2V_EINVAL: a NULL pointer, T / h / w <= 0, threshold outside (0,1), clamp_ratio <= 0, dilate < 0, smooth outside {0,1}, a
 * workspace that is too small, mask not 16-byte aligned, raw / soft / mask_latent overlapping one another. */
int insv2v_automask_finish(const float* raw, float* soft, float* mask_latent, float* mask, void* workspace, int64_t workspace_bytes,
                           int32_t T, int32_t h, int32_t w, float clamp_ratio, float threshold, int32_t smooth, int32_t dilate,
                           insv2v_stream_t stream);

/*
 * ---- a key-frame mask tracked with optical flow (an addition to ABI 15: no existing struct or entry changes) --------------------------
 * One step of the chain that carries a mask drawn on ONE frame k to every frame (csrc/masktrack.hip, DESIGN.md section 19;
 * tests/masktrack_ref.py restates the definition in float64).  The mask is never warped frame by frame: every frame t keeps F_t, the
 * displacement of its pixels to their position in the key frame, and samples the key mask M once.  From the chain's previous frame t'
 * (F_k = 0, V_k = 1) with b = the flow defined on t that points into t' (the convention of insv2v_warp_image: sampling t' at x + b(x)
 * gives t) and, optionally, c = the opposite flow defined on t', per pixel (x, y):
 *   p    = (x + b_x, y + b_y);  inb = 0 <= p_x <= W-1 and 0 <= p_y <= H-1;  pc = p clamped to the frame
 *   S(G) = bilinear sample of G at pc: x0 = floor(pc_x), x1 = min(x0 + 1, W-1), the same in y (border clamp, NOT zero padding), as
 *          lerps: top + ay (bottom - top), top = g00 + ax (g01 - g00) - a constant region is sampled exactly
 *   cons = true when c == NULL, else with cf = S(c), d = b + cf:  |d|^2 <= alpha (|b|^2 + |cf|^2) + beta
 *   Vs   = min of V_prev over the (up to four) neighbours of pc whose bilinear weight is non-zero
 *   F    = b + S(F_prev);   V = inb and cons and Vs > 1/2  (written as 1 / 0)
 *   mask = V ? bilinear sample (border clamp) of M at (x, y) + F, clamped to the frame : fill
 * N chains run in one launch (both directions of a key frame inside the video); all tensors are contiguous fp32.
 * INSV2V_EINVAL: a NULL descriptor or pointer other than c; N <= 0; H <= 1 or W <= 1; alpha or beta negative or not finite; a NaN fill;
 * N*2*H*W beyond the grid; an output that overlaps an input or another output (a pixel reads neighbours that other threads write).
 */
typedef struct insv2v_masktrack_desc {
    const float* f_prev;   /* [N,2,H,W] flow to the key frame of the chain's previous frame */
    const float* v_prev;   /* [N,H,W]   its validity, 0 or 1 */
    const float* b;        /* [N,2,H,W] flow on frame t into t' */
    const float* c;        /* [N,2,H,W] flow on frame t' into t, or NULL: no forward-backward consistency check */
    const float* m;        /* [N,H,W]   the key frame's mask */
    float* f_out;          /* [N,2,H,W] */
    float* v_out;          /* [N,H,W]   */
    float* mask_out;       /* [N,H,W]   */
    int32_t N, H, W;
    float alpha, beta, fill;
} insv2v_masktrack_desc;
int insv2v_mask_track_step(const insv2v_masktrack_desc* d, insv2v_stream_t stream);

/*
 * ---- scoring an edit in pixel space (additions to ABI 15: no existing struct or entry changes) ------------------------------------------
 * The flow warp error of a video (does the edit flicker?) and the per-frame squared error and SSIM between two videos (did the edit leave
 * alone what it should?): csrc/pixel_score.hip; tests/pixel_score_ref.py restates both definitions in float64.
 *
 * Frames are [T,3,H,W] views: fp16, or fp32 with fp32 != 0; element strides for frame, channel and row (all >= 0, row stride >= W), x
 * contiguous - a crop of a larger tensor is a valid operand.  A value is mapped as it is read: v = clamp(x * scale + shift, 0, 1)
 * (0.5, 0.5 for frames in [-1, 1]), so every metric is on [0, 1] data (data_range 1).
 * Reductions have two stages in a fixed order: every workgroup writes its partial sums (fp64) to the caller's workspace, a finalize
 * launch adds them in index order in fp64.  No floating-point atomics: two calls give the same bits.  Nothing is allocated; the
 * workspace (8-byte aligned) holds at least insv2v_*_workspace_bytes bytes.  Outputs are fp64 (8-byte aligned).
 * Host-side conventions, decided by the caller from the sums: mse = sum / weight sum; PSNR = 10 log10(1 / mse), +inf for mse == 0; a
 * region whose weight sum is 0 gives nan.
 */
typedef struct insv2v_frames_view {
    const void* p;
    int64_t stride_t, stride_c, stride_h;
    int32_t fp32;
    float scale, shift;
} insv2v_frames_view;

/* The T-1 adjacent pairs of one video A.  b = fwd[t] is defined on frame t and points into t+1 (the convention of insv2v_warp_image:
 * sampling frame t+1 at x + b(x) gives frame t); c = bwd[t] is the opposite flow.  Per pixel x of frame t, with p, inb, the clamped
 * point and the sample S(.) exactly as defined above for insv2v_mask_track_step (border clamp, lerps):
 *   cons  = true when bwd == NULL, else with cf = S(c), d = b + cf:  |d|^2 <= alpha (|b|^2 + |cf|^2) + beta   (that entry's inequality)
 *   valid = inb and cons
 *   err   = (1/3) sum_c (A_t[c](x) - S(A_{t+1}[c]))^2    fp32: the three squares added in channel order, then divided by 3
 * sums[t] = (sum valid w_t err, sum valid w_t, the count of valid pixels); w = the region weight of frame t, 1 when NULL.  The products
 * w * err are formed and added in fp64.  err_map / valid_map (NULL = not written): err (0 where invalid) and valid as 1 / 0.
 * INSV2V_EINVAL, nothing launched and no output touched: a NULL descriptor, frames, fwd, sums or workspace; T < 2; H <= 1 or W <= 1;
 * alpha or beta negative or not finite; a negative stride or a row stride below W; a workspace that is too small or misaligned; T - 1
 * above 65535 or a plane beyond the grid; an output (sums, maps, workspace) that overlaps an input or another output. */
typedef struct insv2v_warp_error_desc {
    insv2v_frames_view a;
    const float* fwd;      /* [T-1,2,H,W] contiguous */
    const float* bwd;      /* [T-1,2,H,W] contiguous, or NULL: no consistency check */
    const float* w;        /* [T,H,W] contiguous, values in [0,1], or NULL: 1 */
    double* sums;          /* [T-1,3] */
    float* err_map;        /* [T-1,H,W] or NULL */
    float* valid_map;      /* [T-1,H,W] or NULL */
    void* workspace;
    int64_t workspace_bytes;
    int32_t T, H, W;
    float alpha, beta;
} insv2v_warp_error_desc;
/* Bytes of workspace for a video of T frames of H x W; INSV2V_EINVAL for a size the entry refuses. */
int64_t insv2v_warp_error_workspace_bytes(int32_t T, int32_t H, int32_t W);
int insv2v_warp_error(const insv2v_warp_error_desc* d, insv2v_stream_t stream);

/* Source X against edit Y, frame by frame, one pass over the data.  sums[t] (INSV2V_FIDELITY_K fp64 values), w = the region weight
 * (1 when NULL), se = (1/3) sum_c (x - y)^2 per pixel (fp32, as err above):
 *   0 sum se    1 sum w se    2 sum (1-w) se    3 sum w    4 sum (1-w)            each accumulated separately, products in fp64: with a
 *                                                                                  binary w and identical pixels outside, sum 2 is exactly 0
 *   5 sum s     6 sum wc s    7 sum (1-wc) s    8 sum wc   9 sum (1-wc)           over the SSIM centres, wc = w at the window centre
 * SSIM (Wang et al. 2004): Gaussian window of 11 taps, sigma 1.5, weights exp(-k^2 / 2 sigma^2), k = -5..5, normalised to sum 1,
 * separable; the window stays inside the frame - centres 5 <= y <= H-6, 5 <= x <= W-6, no padding; C1 = 0.01^2, C2 = 0.03^2;
 * population (co)variances sx2 = E[x^2] - mx^2, sxy = E[xy] - mx my; per channel
 *   ((2 mx my + C1) (2 sxy + C2)) / ((mx^2 + my^2 + C1) (sx2 + sy2 + C2)),   s = the mean of the three channels at a centre.
 * fp32: the moments are those of x - 1/2 and y - 1/2 (the variances do not change, their cancellation error shrinks), a row pass then a
 * column pass, each a sum in tap order.
 * INSV2V_EINVAL: as insv2v_warp_error (T < 1 in place of T < 2, no alpha / beta), and H < 11 or W < 11. */
#define INSV2V_FIDELITY_K 10
typedef struct insv2v_fidelity_desc {
    insv2v_frames_view x, y;
    const float* w;        /* [T,H,W] contiguous, values in [0,1], or NULL: 1 */
    double* sums;          /* [T,INSV2V_FIDELITY_K] */
    void* workspace;
    int64_t workspace_bytes;
    int32_t T, H, W;
} insv2v_fidelity_desc;
int64_t insv2v_frame_fidelity_workspace_bytes(int32_t T, int32_t H, int32_t W);
int insv2v_frame_fidelity(const insv2v_fidelity_desc* d, insv2v_stream_t stream);
/* The kernel's tile of SSIM centres (rows, columns): what the tests name their shapes from.  Returns 0. */
int insv2v_frame_fidelity_tile(int32_t* rows, int32_t* cols);

/*
 * ---- stabilizing an edit along the source video's flow (an addition to ABI 15: no existing struct or entry changes) ---------------------
 * A temporal filter on decoded frames (csrc/temporal_filter.hip; tests/temporal_filter_ref.py restates the
 * definition in float64).  E [T,3,H,W] is the edit, read as it is; A is the guide (the SOURCE video), read as a = clamp(x * scale +
 * shift, 0, 1) like every insv2v_frames_view.  Neighbour k of frame t is frame t + offsets[k]; G_{t,k} = flow[k][t] is defined on frame t
 * and points into that frame (the convention of insv2v_warp_image), U_{t,k} = valid[k][t] is 1 where the trajectory may be followed.
 * A neighbour outside the video, or with U <= 1/2, is SKIPPED (its G, E and A are not read: a NaN there cannot leak).  For the others,
 * in the order k = 0 .. K-1, with p = x + G(x), its clamp and the sample S(.) exactly as defined for insv2v_mask_track_step:
 *   d2  = (1/3) sum_c (a_t[c](x) - S(a_{t+k}[c]))^2          fp32: the three squares added in channel order, then divided by 3
 *   w_k = strength * expf(d2 * (-1 / (2 sigma^2)))             the factor is formed in double on the host and rounded once
 *   out_t[c](x) = E_t[c](x) + (sum_k w_k (S(E_{t+k}[c]) - E_t[c](x))) / (1 + sum_k w_k)
 * and out = E_t[c](x), its own bits, when that quotient is 0: a pixel without a valid neighbour and a video that is constant along its
 * trajectories come back bit for bit.  All arithmetic is fp32; the output has E's dtype and is rounded once, on the store.  Every thread
 * writes its own pixel: no atomics, two calls give the same bits.  Nothing is allocated.
 * INSV2V_EINVAL, nothing launched and no output touched: a NULL descriptor or pointer; T < 1; K outside 1 .. INSV2V_TFILTER_MAX_K; an
 * offset that is 0 or beyond +-INSV2V_TFILTER_MAX_RADIUS; H <= 1 or W <= 1; sigma not finite or <= 0; strength outside (0, 1]; a guide
 * affine that is not finite; a negative stride or a row stride below W; T above 65535 or a plane beyond the grid; an output that
 * overlaps E, A, flow or valid (a pixel reads other frames that other threads write).
 */
#define INSV2V_TFILTER_MAX_K 8
#define INSV2V_TFILTER_MAX_RADIUS 4
typedef struct insv2v_temporal_filter_desc {
    insv2v_frames_view e;    /* the edit; scale / shift are not read */
    insv2v_frames_view a;    /* the guide */
    const float* flow;       /* [K,T,2,H,W] contiguous */
    const float* valid;      /* [K,T,H,W] contiguous, 0 or 1 */
    void* out;               /* [T,3,H,W] of E's dtype, element strides below, x contiguous */
    int64_t out_stride_t, out_stride_c, out_stride_h;
    int32_t offsets[INSV2V_TFILTER_MAX_K];
    int32_t K, T, H, W;
    float sigma, strength;
} insv2v_temporal_filter_desc;
int insv2v_temporal_filter(const insv2v_temporal_filter_desc* d, insv2v_stream_t stream);

/*
 * ---- filling the frames between edited key frames (an addition to ABI 15: no existing struct or entry changes) ---------------------------
 * Only every N-th frame of a video is denoised; the frames in between take the edit from their neighbouring key frames along the SOURCE
 * video's motion (csrc/keyfill.hip; tests/keyfill_ref.py restates the definition in float64).
 * A [T,3,H,W] is the source video: its raw values x are used for the residual and the result, a = clamp(x * scale + shift, 0, 1) for
 * the photometric weight, exactly as insv2v_temporal_filter reads its guide.  E [Tk,3,H,W] holds the edited key frames (scale / shift
 * are not read); key slot j is frame key_frame[j] of A.  Entry i of the frame table is the in-between frame t = frame[i] with up to two
 * sides, s = 0 (the previous key) and s = 1 (the next key): slot[i][s] is the side's key slot (-1: the side does not exist),
 * weight[i][s] = tw_s >= 0 its temporal weight (tw_0 + tw_1 = 1 over the existing sides), G_s = flow[i][s] is defined on frame t and
 * points into the key's frame (the convention of insv2v_warp_image) and U_s = valid[i][s] is 1 where that trajectory may be followed.
 * A side is ACTIVE at pixel x when its slot is >= 0 and U_s(x) > 1/2.  An inactive side's G, and the taps it would reach, are not
 * read: a NaN there cannot leak.  Per active side, in the order s = 0, 1, with p = x + G_s(x), its clamp and the sample S(.) exactly
 * as defined for insv2v_mask_track_step (mt_taps / mt_lerp of csrc/flow_sample.h):
 *   d2_s   = (1/3) sum_c (a_t[c](x) - S(a_key[c]))^2          fp32: the three squares added in channel order, then divided by 3
 *   w_s    = tw_s * expf(d2_s * (-1 / (2 sigma^2)))           the factor is formed in double on the host and rounded once
 *   r_s[c] = S(E_key[c] - A_key[c])                           mode INSV2V_KEYFILL_RESIDUAL: the lerp over the four per-tap differences,
 *                                                             each formed in fp32 with A raw - exactly 0 when E == A in all four taps
 *   r_s[c] = S(E_key[c]) - A_t[c](x)                          mode INSV2V_KEYFILL_WARP
 * With Wsum = sum of w_s over the active sides:
 *   Wsum > 0:   out[c] = A_t[c](x) + (sum_s w_s r_s[c]) / Wsum,  conf(x) = Wsum (in (0, 1])
 *   otherwise (a hole: no active side, or every weight underflowed):
 *               out[c] = A_t[c](x) + sum over the sides with slot >= 0 of tw'_s r0_s[c],  conf(x) = 0
 *               r0_s = the same quantity taken at x itself, no flow read; tw' = tw renormalised over the existing sides (formed in
 *               double on the host, rounded once)
 * and out = A_t[c](x) itself, converted once to the output dtype, when the added term q is 0 (q == 0.f): where the edit changed
 * nothing in the taps of its keys the in-between pixel is the source's - bit for bit when A and the output share a dtype.
 * All arithmetic is fp32; the output has E's dtype and is rounded once, on the store.  `out` is the FULL-RATE tensor [T,3,H,W]: only
 * the frames of the table are written, the key frames' rows are not touched.  conf [n,H,W] fp32 may be NULL.  One thread writes one
 * pixel: no atomics, two calls give the same bits.  Nothing is allocated, nothing is copied to the device and nothing synchronises (the
 * tables are HOST arrays, validated here and passed to the kernel by value in launches of at most INSV2V_KEYFILL_MAX_FRAMES frames),
 * so the call can be captured.
 * INSV2V_EINVAL, nothing launched and no output touched: a NULL descriptor or required pointer; n < 1, Tk < 1 or T < 1; H <= 1 or
 * W <= 1; a frame or key_frame[j] outside 0 .. T-1; a frame listed twice or equal to a key frame; a slot outside -1 .. Tk-1; both
 * slots -1; a weight that is negative or not finite, or whose existing sides do not sum to 1 within 1e-6; sigma not finite or <= 0
 * (or 2 sigma^2 underflowing); a mode other than 0 / 1; a guide affine that is not finite; a negative stride or a row stride below W;
 * T or Tk above 65535 or a plane beyond the grid (the limits of insv2v_temporal_filter); an output or conf that overlaps any input or
 * each other.
 */
#define INSV2V_KEYFILL_MAX_FRAMES 64
#define INSV2V_KEYFILL_RESIDUAL 0
#define INSV2V_KEYFILL_WARP 1
typedef struct insv2v_keyfill_desc {
    insv2v_frames_view a;      /* the source video [T,3,H,W] */
    insv2v_frames_view e;      /* the edited key frames [Tk,3,H,W]; scale / shift are not read */
    const float* flow;         /* [n,2,2,H,W] contiguous: frame, side, (x, y) */
    const float* valid;        /* [n,2,H,W] contiguous, 0 or 1 */
    void* out;                 /* [T,3,H,W] of E's dtype, element strides below, x contiguous */
    int64_t out_stride_t, out_stride_c, out_stride_h;
    float* conf;               /* [n,H,W] contiguous, or NULL */
    const int32_t* key_frame;  /* HOST [Tk] */
    const int32_t* frame;      /* HOST [n] */
    const int32_t* slot;       /* HOST [n,2] */
    const float* weight;       /* HOST [n,2] */
    int32_t n, T, Tk, H, W, mode;
    float sigma;
} insv2v_keyfill_desc;
int insv2v_keyframe_fill(const insv2v_keyfill_desc* d, insv2v_stream_t stream);

/*
 * ---- growing, shrinking and feathering a mask (an addition to ABI 15: no existing struct or entry changes) --------------------------------
 * A mask m [T,H,W] fp32 from any source becomes the two masks a localized edit wants (csrc/mask_shape.hip, DESIGN.md section 22;
 * tests/mask_shape_ref.py restates the definition with integers and float64): `shaped`, soft, for the pixel composite, and `support`,
 * hard and covering the whole feather, for the latent hold.  Parameters: threshold tau, grow g (pixels, negative shrinks), feather
 * f >= 0 (pixels), profile (INSV2V_MASK_PROFILE_*).  Per frame:
 *   inside   = m > tau (strict; a NaN is outside)
 *   D2_out(x) = the squared Euclidean distance from x to the nearest inside pixel of the frame (0 on inside pixels);
 *   D2_in(x)  = the same to the nearest outside pixel (0 on outside pixels).  Both are integers.  The frame border is NOT outside: a
 *               mask that touches it stays full up to it.  R = ceil(max(g + f, 1 - g, 1)) is the smallest search radius that decides
 *               every pixel; every D2 > R^2 - also that of a frame without any inside (outside) pixel - is FAR = (R + 1)^2.
 *   s(x)     = sqrt(D2_out) on outside pixels (>= 1),  1 - sqrt(D2_in) on inside pixels (<= 0): the signed distance to the edge
 *   shaped   = 1 where s <= g;  else 0 where s >= g + f;  else, with u = (g + f - s) / f, u (linear) or u^2 (3 - 2 u) (smooth), kept
 *              inside [2^-126, 1 - 2^-24] so that a ramp value is never exactly 0 or 1.  The feather lies OUTSIDE the grown edge.
 *   support  = 1 where shaped > 0, else 0.
 * The two hard decisions are taken on integers: D2 against the four thresholds of insv2v_mask_shape_plan, which are the comparisons on
 * s in float64 turned into integers (floor(g^2), ceil((g + f)^2) and their mirrors (1 - g)^2, (1 - g - f)^2 wherever those squares are
 * exact).  So exactly 1, exactly 0 and support are exact; only the ramp is floating point - fp32, in this order: s from sqrtf of the
 * integer, u = (gf - s) / f with gf = g + f formed in double and rounded once, then u * u * (3 - 2 u).
 * Limits: -32 <= g <= 32, 0 <= f <= 32, g + f >= -32 (INSV2V_MASK_SHAPE_MAX), so R <= 64.
 * Two launches: a column pass writes, per pixel, the capped vertical distance to the nearest inside / outside pixel of its column into
 * the workspace (one signed byte), a row pass takes min over |dx| <= R of dx^2 + v(x + dx)^2 in int32 from LDS, decides and stores.
 * Every thread writes its own pixels with plain stores: no atomics, two calls give the same bits.  Nothing is allocated: the caller
 * passes workspace (4-byte aligned) of at least insv2v_mask_shape_workspace_bytes(T,H,W) bytes.  d2_out / d2_in (NULL = not written)
 * return the two integer maps.
 * INSV2V_EINVAL, nothing launched and no output touched: a NULL descriptor, m, shaped, support or workspace; T, H or W < 1, or more row
 * tiles than a grid holds; g or f outside the limits or not finite; tau not finite; a profile outside {0, 1}; a workspace that is too
 * small or misaligned; an output (shaped, support, d2_out, d2_in, workspace) that overlaps m or another output.
 */
#define INSV2V_MASK_SHAPE_MAX 32
#define INSV2V_MASK_PROFILE_LINEAR 0
#define INSV2V_MASK_PROFILE_SMOOTH 1
typedef struct insv2v_mask_shape_plan_t {
    int32_t rc;          /* 0, or INSV2V_EINVAL for (grow, feather) the entry refuses: every other field is then meaningless */
    int32_t R;           /* search radius */
    int32_t far;         /* (R + 1)^2 */
    int32_t out_one;     /* outside pixel: shaped = 1  iff D2_out <= out_one   (-1: never) */
    int32_t out_zero;    /*                shaped = 0  iff D2_out >= out_zero, checked after out_one */
    int32_t in_one;      /* inside pixel:  shaped = 1  iff D2_in >= in_one */
    int32_t in_zero;     /*                shaped = 0  iff D2_in <= in_zero    (-1: never), checked after in_one */
    int32_t row_tile;    /* pixels of a row one workgroup of the row pass owns: what the tests place their blobs by */
} insv2v_mask_shape_plan_t;
/* Host-only, launches nothing; returns out->rc (INSV2V_EINVAL also for out == NULL). */
int insv2v_mask_shape_plan(float grow, float feather, insv2v_mask_shape_plan_t* out);
typedef struct insv2v_mask_shape_desc {
    const float* m;        /* [T,H,W] */
    float* shaped;         /* [T,H,W] */
    float* support;        /* [T,H,W] */
    int32_t* d2_out;       /* [T,H,W] or NULL */
    int32_t* d2_in;        /* [T,H,W] or NULL */
    void* workspace;
    int64_t workspace_bytes;
    int32_t T, H, W;
    float threshold, grow, feather;
    int32_t profile;
} insv2v_mask_shape_desc;
/* Bytes of workspace for a [T,H,W] mask; INSV2V_EINVAL for a size the entry refuses. */
int64_t insv2v_mask_shape_workspace_bytes(int32_t T, int32_t H, int32_t W);
int insv2v_mask_shape(const insv2v_mask_shape_desc* d, insv2v_stream_t stream);

/*
 * ---- editing a region at full resolution (additions to ABI 15: no existing struct or entry changes) ------------------------------------------
 * The box around a mask is resampled to the model's working size, edited there, and what the edit changed is resampled back and laid
 * over the untouched full-resolution source (csrc/region.hip; tests/region_ref.py restates the definition in
 * float64).  All operands are fp32; views have element strides and contiguous rows, so a crop of a larger tensor is a valid operand.
 *
 * RESAMPLING is the separable antialiased resampling of torch.nn.functional.interpolate(antialias=True, align_corners=False) applied
 * to the CROP.  Per axis, with n_in source and n_out destination samples: scale = n_in / n_out, s = max(scale, 1); for destination
 * index i: c = scale (i + 0.5), xmin = max(int(c - support s + 0.5), 0), xsize = min(int(c + support s + 0.5), n_in) - xmin, weights
 * f((j + xmin - c + 0.5) / s) for j < xsize, divided by their sum.  INSV2V_REGION_BICUBIC: the cubic convolution with A = -0.5,
 * support 2; INSV2V_REGION_BILINEAR: the triangle, support 1.  The taps are clipped at the edges of the BOX, not of the frame.  c and the
 * tap range are formed in double, the weights in fp32 and normalised by their sum in tap order; the horizontal pass comes first, every
 * output is an fp32 fma chain in tap order.  With n_in == n_out the weights are exactly 0, 1, 0, 0: an equal-size box is copied bit
 * for bit.  One launch for all frames and channels, no intermediate image in HBM, no atomics: two calls give the same bits.
 * Every entry returns INSV2V_EINVAL before any launch, and leaves its outputs untouched, for: a NULL descriptor or required pointer; a
 * size that is not positive (or a side above 2^24, a box or working height above 16 * 65535, or more than 65535 planes n * C); a box that is empty or not inside the frame; a
 * per-axis ratio box / working size outside [1/8, 8] (what bounds the kernels' LDS staging); an unknown filter or mode; a negative
 * stride or a row stride below W; an output that overlaps an input.
 */
#define INSV2V_REGION_BICUBIC 0
#define INSV2V_REGION_BILINEAR 1
#define INSV2V_REGION_RESIDUAL 0
#define INSV2V_REGION_REPLACE 1
/* boxes[T + 1][4] int32: per frame of the mask view [T,H,W] (stride_t may be 0: one mask for every frame) and, in entry T, over all
 * frames, the half-open box (x0, y0, x1, y1) of the pixels with mask > threshold (strict; a NaN is outside); a frame without one gives
 * (W, H, 0, 0).  The entry initialises boxes itself (two launches); the reduction ends in integer min / max atomics, which commute:
 * the result is a function of the inputs only.  Also INSV2V_EINVAL: T above 65534, a threshold that is not finite. */
int insv2v_mask_bbox(const float* mask, int64_t stride_t, int64_t stride_h, int32_t T, int32_t H, int32_t W, float threshold,
                     int32_t* boxes, insv2v_stream_t stream);
/* dst[n,C,h,w] = resample(src[n,C, y0:y1, x0:x1] -> (h, w)) with `filter`; clamp != 0: then clamped to [clamp_lo, clamp_hi] (a NaN
 * stays a NaN).  Also INSV2V_EINVAL: clamp outside {0, 1}, clamp_lo > clamp_hi. */
typedef struct insv2v_region_resample_desc {
    const float* src;          /* [n,C,H,W] view */
    int64_t src_stride_n, src_stride_c, src_stride_h;
    float* dst;                /* [n,C,h,w] contiguous */
    int32_t n, C, H, W, h, w;
    int32_t x0, y0, x1, y1;    /* the box, half-open, inside the frame */
    int32_t filter, clamp;
    float clamp_lo, clamp_hi;
} insv2v_region_resample_desc;
int insv2v_region_resample(const insv2v_region_resample_desc* d, insv2v_stream_t stream);
/* The paste.  `out` [n,C,H,W] holds the SOURCE (the caller hands in a clone); only the box is written, and a pixel is read before it is
 * written, by the same thread.  ramp(x, y) = min(1, (d + 0.5) / blend), d = the distance in pixels to the nearest box edge that is not
 * also a frame border (1 when blend == 0, or when no such edge exists).  With U(.) the bicubic and V(.) the bilinear resampling of a
 * working-resolution [h,w] image to the box:
 *   INSV2V_REGION_RESIDUAL:  out = clip(src + ramp U(edit - down), -1, 1)     the difference is formed in fp32 as the operand is loaded:
 *                            where edit == down in all of a pixel's taps the added term is exactly 0 and the pixel keeps the source's value
 *   INSV2V_REGION_REPLACE:   out = clip(src + M (U(edit) - src), -1, 1),  M = ramp clamp(V(mask), 0, 1), M = ramp when mask == NULL;
 *                            `down` is not read
 * In both modes a pixel whose added term is exactly 0 (0.f == the term) keeps the source's own bits, also those of a -0, before the clip.
 * mask [n,h,w] has rows of w and planes of h * w; mask_stride_n is the frame stride (0: one mask for every frame).  Also
 * INSV2V_EINVAL: down == NULL in residual mode; a blend that is negative or not finite; a mask stride below h * w other than 0. */
typedef struct insv2v_region_paste_desc {
    const float* edit;         /* [n,C,h,w] contiguous: the edited working clip */
    const float* down;         /* [n,C,h,w] contiguous: the working clip the edit started from (residual mode) */
    const float* mask;         /* [n,h,w] or NULL (replace mode) */
    int64_t mask_stride_n;
    float* out;                /* [n,C,H,W] view */
    int64_t out_stride_n, out_stride_c, out_stride_h;
    int32_t n, C, H, W, h, w;
    int32_t x0, y0, x1, y1;
    int32_t mode;
    float blend;
} insv2v_region_paste_desc;
int insv2v_region_paste(const insv2v_region_paste_desc* d, insv2v_stream_t stream);

/*
 * ---- a region that follows the object: one real-valued box per frame (additions to ABI 15: no existing struct or entry changes) -----------
 * The two entries above with a TRACK in place of the box: n boxes (x0, y0, x1, y1) of doubles, one per frame, read on the HOST
 * (csrc/region.hip; tests/region_track_ref.py restates the definition in float64).  A box is half-open in continuous
 * pixel coordinates - pixel j covers [j, j + 1), its centre is j + 0.5 - finite, with x1 > x0 and y1 > y0, inside [0, W] x [0, H].  A
 * frame's COVER is the integer box [floor(x0), ceil(x1)) x [floor(y0), ceil(y1)).
 *
 * RESAMPLE (box -> working size), per axis: n_out destination samples, e = x1 - x0, X0 = floor(x0), n_in = ceil(x1) - X0,
 * scale = e / n_out, s = max(scale, 1), and for destination index i the centre in cover coordinates c = (x0 - X0) + scale (i + 0.5);
 * the tap range and the weights are those of the entries above with this c and this n_in.  The taps are clipped at the COVER: the
 * working clip depends on the cover's pixels only, and for an integer box (cover = box, x0 - X0 = 0.0, e = n_in) the operator is the one
 * above, bit for bit.  A consequence: as x0 crosses an integer the cover gains or loses a column, and the outputs within support s of
 * that edge change discontinuously, by a renormalisation; those pixels lie under the paste's ramp.
 *
 * PASTE (working size -> each frame's cover), per axis: the source is the working image of n_w samples, scale' = n_w / e,
 * s = max(scale', 1), c = scale' (X + 0.5 - x0) for the cover's pixel X; taps clipped to [0, n_w) and normalised.
 * ramp = clamp(d / blend, 0, 1), d = the distance from the pixel's centre to the nearest box edge that is not a frame border (negative
 * outside the box); an edge is a frame border only when x0 == 0, x1 == W, y0 == 0 or y1 == H exactly; blend == 0: 1 where the centre
 * lies inside the box, else 0; no such edge: 1.  For an integer box this is min(1, (d_int + 0.5) / blend).  The modes, the operand formed
 * as it is loaded, add == 0 ? src : src + add, the mask resampled bilinearly and clamped to [0, 1], the final clip and the read before the
 * write by the same thread are those of insv2v_region_paste; only the cover is written, and a pixel whose ramp is 0 keeps the source
 * (what was resampled for it is not used).
 *
 * The boxes travel to the kernels by value, in launches of at most 64 frames (2 KiB of arguments): no device buffer, no allocation,
 * no synchronisation.  Every output is a sum in tap order by one thread: two calls give the same bits.  INSV2V_EINVAL before the first
 * launch, outputs untouched: everything the entries above refuse; boxes == NULL; a coordinate that is not finite; an empty box; a box
 * outside the frame; a per-axis ratio e / working size outside [1/8, 8] for any frame.
 */
typedef struct insv2v_region_resample_track_desc {
    const float* src;          /* [n,C,H,W] view */
    int64_t src_stride_n, src_stride_c, src_stride_h;
    float* dst;                /* [n,C,h,w] contiguous */
    const double* boxes;       /* HOST pointer, [n][4]: (x0, y0, x1, y1) per frame */
    int32_t n, C, H, W, h, w;
    int32_t filter, clamp;
    float clamp_lo, clamp_hi;
} insv2v_region_resample_track_desc;
int insv2v_region_resample_track(const insv2v_region_resample_track_desc* d, insv2v_stream_t stream);
typedef struct insv2v_region_paste_track_desc {
    const float* edit;         /* [n,C,h,w] contiguous */
    const float* down;         /* [n,C,h,w] contiguous (residual mode) */
    const float* mask;         /* [n,h,w] or NULL (replace mode) */
    int64_t mask_stride_n;
    float* out;                /* [n,C,H,W] view: holds the source, only each frame's cover is written */
    int64_t out_stride_n, out_stride_c, out_stride_h;
    const double* boxes;       /* HOST pointer, [n][4] */
    int32_t n, C, H, W, h, w;
    int32_t mode;
    float blend;
} insv2v_region_paste_track_desc;
int insv2v_region_paste_track(const insv2v_region_paste_track_desc* d, insv2v_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* INSV2V_HIP_H */
