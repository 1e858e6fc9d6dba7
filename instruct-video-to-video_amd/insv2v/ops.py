"""Thin tensor-level wrappers over the C ABI (one Python call = one kernel family launch).

PyTorch is plumbing here: device memory (torch.empty), the current HIP stream, and nothing
else.  No op has a torch/CPU fallback; non-CUDA tensors are rejected.
"""
import ctypes as C

import math
import os
import torch

from . import _lib
from .rng import as_int64
from ._lib import GemmDesc, GroupNormDesc, LayerNormDesc, AttentionDesc, StepDesc, MStepDesc, MaskStepDesc, RelStepDesc, MaskTrackDesc, FfnDesc, RowLinDesc, TattnDesc, XattnDesc, WinogradInDesc, WinogradOutDesc, check

ACT_NONE, ACT_SILU, ACT_GEGLU, ACT_QUICK_GELU = 0, 1, 2, 3
ACT_RELU, ACT_SIGMOID, ACT_TANH = 4, 5, 6   # the optical-flow network's (insv2v/raft.py)
EW_RELU, EW_ADD_RELU, EW_TANH, EW_GRU_RH, EW_GRU_OUT = 1, 2, 3, 4, 5
_byref = C.byref


def _stream():
    return torch.cuda.current_stream().cuda_stream


# Optional per-launch timing (bench.py roofline leg): list of (kernel family, algorithmic flops, ev0, ev1)
# with HIP events recorded on the launch stream.  None = no overhead.
_REC = None


def set_launch_recorder(rec):
    global _REC
    _REC = rec


class _timed:
    __slots__ = ("name", "work", "e0", "tag")

    def __init__(self, name, work, tag=None):
        self.name, self.work, self.tag = name, work, tag

    def __enter__(self):
        if _REC is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record()

    def __exit__(self, *exc):
        if _REC is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            _REC.append((self.name, self.work, self.e0, e1) if self.tag is None else (self.name, self.work, self.e0, e1, self.tag))
        return False


def _ptr(t):
    return t.data_ptr() if t is not None else None


def _req(t, dtype, name):
    if not torch.is_tensor(t):
        raise _lib.HipKernelError(f"{name}: expected a CUDA {dtype} tensor, got {type(t).__name__}")
    if not (t.is_cuda and t.dtype == dtype):
        raise _lib.HipKernelError(f"{name}: expected a CUDA {dtype} tensor, got {t.device} {t.dtype}")
    return t


_WORKSPACE = {}
_WS_OVERRIDE = None
WORKSPACE_BYTES = 64 << 20


def new_workspace(device):
    """fp32 split-K scratch.  A captured hipGraph must own the scratch its kernels point at: GraphedUNet allocates one
    per concurrent branch BEFORE capture and installs it with ``workspace(...)`` (a scratch allocated lazily inside a
    capture would live in that graph's private memory pool while being cached here for other graphs)."""
    return torch.empty(WORKSPACE_BYTES // 4, device=device, dtype=torch.float32)


class workspace:
    """Context manager: launches inside use ``ws`` as their split-K scratch (one per concurrently running stream)."""

    def __init__(self, ws):
        self.ws = ws

    def __enter__(self):
        global _WS_OVERRIDE
        self.prev, _WS_OVERRIDE = _WS_OVERRIDE, self.ws

    def __exit__(self, *exc):
        global _WS_OVERRIDE
        _WS_OVERRIDE = self.prev
        return False


def _workspace(device):
    """The installed scratch, else a persistent one per (device, stream): launches on one stream are serialised, so
    sharing within a stream is safe."""
    if _WS_OVERRIDE is not None:
        return _WS_OVERRIDE
    key = (device, torch.cuda.current_stream().cuda_stream)
    ws = _WORKSPACE.get(key)
    if ws is None:
        ws = _WORKSPACE[key] = new_workspace(device)
    return ws


class RowStats:
    """LayerNorm statistics of a token matrix as the PRODUCING GEMM left them: ``parts`` [nparts, M, 2] fp32 partial
    (sum, sum of squares) per column tile (gemm(..., emit_stats=True)), finalised by the consumer (gemm(row_stats=RowStats))."""
    __slots__ = ("parts", "nparts", "eps")

    def __init__(self, parts, nparts, eps):
        self.parts, self.nparts, self.eps = parts, nparts, eps


_STATS_PARTS_CACHE = {}


def gemm(a, w, bias=None, *, a2=None, act=ACT_NONE, residual=None, row_bias=None, rows_per_group=0, rb_mod=0,
         row_stats=None, col_sum=None, emit_stats=False, ln_eps=1e-5,
         out=None, out_fp32=False, alpha=1.0, tile=0, split_k=0, batch=1, a_bs=0, w_bs=0, c_bs=0, r_bs=0,
         M=None, N=None, K=None, lda=None, ldw=None, ldc=None):
    """out[M,N'] = epilogue(alpha * [a|a2] @ w^T); see insv2v_gemm in include/insv2v_hip.h."""
    lib = _lib.load()
    _req(a, torch.float16, "gemm.a"), _req(w, torch.float16, "gemm.w")
    M = a.shape[0] if M is None else M
    N = w.shape[0] if N is None else N
    k1 = a.shape[1]
    K = (k1 + (a2.shape[1] if a2 is not None else 0)) if K is None else K
    n_out = N // 2 if act == ACT_GEGLU else N
    if out is None:
        shape = (M, n_out) if batch == 1 else (batch, M, n_out)
        out = torch.empty(shape, device=a.device, dtype=torch.float32 if out_fp32 else torch.float16)
    d = GemmDesc()
    d.a, d.w, d.c = a.data_ptr(), w.data_ptr(), out.data_ptr()
    d.lda = a.stride(0) if lda is None else lda
    d.ldw = w.stride(0) if ldw is None else ldw
    d.ldc = (out.stride(-2) if ldc is None else ldc)
    if a2 is not None:
        _req(a2, torch.float16, "gemm.a2")
        d.a2, d.lda2, d.k_split = a2.data_ptr(), a2.stride(0), k1
    if bias is not None:
        d.bias = _req(bias, torch.float32, "gemm.bias").data_ptr()
    if row_bias is not None:
        d.row_bias, d.ld_rb, d.rows_per_group = _req(row_bias, torch.float32, "gemm.row_bias").data_ptr(), row_bias.stride(0), rows_per_group
    if residual is not None:
        d.residual, d.ldr = _req(residual, torch.float16, "gemm.residual").data_ptr(), residual.stride(-2)
    scratch = None
    if isinstance(row_stats, RowStats):
        d.row_stats = row_stats.parts.data_ptr()
        d.stats_parts, d.ln_eps = row_stats.nparts, row_stats.eps
        scratch = torch.empty((M, 2), device=a.device, dtype=torch.float32)  # only touched by kernels that park (mean, rstd); held until the launch
        d.stats_scratch = scratch.data_ptr()
        d.col_sum = _req(col_sum, torch.float32, "gemm.col_sum").data_ptr()
    elif row_stats is not None:
        d.row_stats = _req(row_stats, torch.float32, "gemm.row_stats").data_ptr()
        d.col_sum = _req(col_sum, torch.float32, "gemm.col_sum").data_ptr()
    d.rb_mod = rb_mod
    d.M, d.N, d.K, d.act, d.c_fp32, d.alpha, d.tile = M, N, K, act, int(out.dtype == torch.float32), alpha, tile
    d.batch, d.a_bs, d.w_bs, d.c_bs, d.r_bs = batch, a_bs, w_bs, c_bs, r_bs
    if batch == 1:
        ws = _workspace(a.device)
        d.workspace, d.workspace_bytes, d.split_k = ws.data_ptr(), ws.numel() * 4, split_k
    stats = None
    if emit_stats:
        # statistics of the rows just produced, for the LayerNorm that consumes them (one pair per column tile of the kernel the
        # library picks for this problem; problems it cannot instrument fall back to the statistics pass over the output)
        key = (M, N, K, d.lda, d.ldc, d.ldr, residual is not None, act, tile, out.dtype, a.data_ptr() % 16, out.data_ptr() % 16, batch, split_k,
               residual.data_ptr() % 16 if residual is not None else 0,
               # the dispatch (pick_pingpong: 160-column parts on gemm_r8, 128 on the 128x128 tile) also looks at these
               row_bias is not None, rows_per_group, d.ld_rb, rb_mod, a2 is not None, row_stats is not None)
        nparts = _STATS_PARTS_CACHE.get(key)
        if nparts is None:
            nparts = _STATS_PARTS_CACHE[key] = int(lib.insv2v_gemm_stats_parts(_byref(d)))
        if nparts > 0:
            stats = RowStats(torch.empty((nparts, M, 2), device=a.device, dtype=torch.float32), nparts, ln_eps)
            d.stats_out = stats.parts.data_ptr()
    with _timed("gemm_kernel", 2.0 * M * N * K * batch, ("lin", M, N, K, batch, act, residual is not None)):
        rc = lib.insv2v_gemm(_byref(d), _stream())
        if rc == -2 and stats is not None:   # documented behaviour: a problem that cannot emit statistics gets the statistics pass
            stats, d.stats_out = None, None
            rc = lib.insv2v_gemm(_byref(d), _stream())
        check(rc, "insv2v_gemm")
    del scratch
    if emit_stats:
        return out, (stats if stats is not None else layernorm_stats(out, ln_eps))
    return out


def copy_rows(dst, src):
    """dst <- src (a device-to-device copy of token rows on the current stream), visible to the launch recorder like any other launch:
    the duplicated CFG-branch rows of unet.forward_cl(cfg_clips=...)."""
    with _timed("copy", 0.0, ("copy", src.shape[0], src.shape[1])):
        dst.copy_(src)
    return dst


def ffn_fused_supported(C, hidden):
    """True if insv2v_ffn_fused handles this width (the register-resident kernel exists for C = 320, hidden = 1280)."""
    return int(_lib.load().insv2v_ffn_stream_elems(C, hidden, 0)) > 0


def ffn_fused(x, wstream, hidden, eps=1e-5, out=None, post_residual=None):
    """out = x + FeedForward_geglu(LayerNorm(x)) in one launch (insv2v_ffn_fused); wstream from fused.pack_ffn_stream.
    post_residual: the stream also carries the module's trailing Linear (pack_ffn_stream(post=...)):
    out = Wp (x + FF(LN(x))) + bp + post_residual."""
    lib = _lib.load()
    _req(x, torch.float16, "ffn.x"), _req(wstream, torch.float16, "ffn.wstream")
    M, C = x.shape
    if wstream.numel() != int(lib.insv2v_ffn_stream_elems(C, hidden, int(post_residual is not None))):
        raise _lib.HipKernelError(f"ffn_fused: weight stream of {wstream.numel()} halfs does not match C={C}, hidden={hidden}, post={post_residual is not None}")
    if out is None:
        out = torch.empty((M, C), device=x.device, dtype=torch.float16)
    d = FfnDesc()
    d.x, d.out, d.wstream, d.ldx, d.ldo = x.data_ptr(), out.data_ptr(), wstream.data_ptr(), x.stride(0), out.stride(0)
    d.M, d.C, d.hidden, d.eps = M, C, hidden, eps
    if post_residual is not None:
        d.post, d.post_residual, d.ld_post = 1, _req(post_residual, torch.float16, "ffn.post_residual").data_ptr(), post_residual.stride(0)
    with _timed("gemm_kernel", 2.0 * M * C * 3 * hidden + (2.0 * M * C * C if post_residual is not None else 0.0), ("ffn", M, C, hidden)):
        check(lib.insv2v_ffn_fused(_byref(d), _stream()), "insv2v_ffn_fused")
    return out


def rowlin_supported(N, K):
    """True if insv2v_rowlin handles a [N, K] Linear (K = 320 or 640, N a multiple of 64)."""
    return int(_lib.load().insv2v_rowlin_stream_elems(N, K)) > 0


def rowlin(x, wstream, N, *, layernorm=False, residual=None, frames=0, rows_per_frame=0, eps=1e-5, out=None, emit_stats=False, stats_eps=1e-5,
           gn_ab=None, gn_rows=0):
    """out = [LayerNorm](x) W^T + bias [+ residual] on the register-resident kernel (insv2v_rowlin); wstream from
    fused.pack_linear_stream (frames > 0: it carries a per-frame bias table and row m uses frame (m // rows_per_frame) % frames).
    gn_ab (groupnorm_stats) with gn_rows: the GroupNorm of row m's sample m // gn_rows is applied to x on the fly; every gn_rows > 0
    (a sample's rows go in 32-row wave blocks of its own, fused.row_units)."""
    lib = _lib.load()
    _req(x, torch.float16, "rowlin.x"), _req(wstream, torch.float16, "rowlin.wstream")
    M, K = x.shape
    if wstream.numel() != int(lib.insv2v_rowlin_stream_elems(N, K)):
        raise _lib.HipKernelError(f"rowlin: weight stream of {wstream.numel()} halfs does not match N={N}, K={K}")
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float16)
    d = RowLinDesc()
    d.x, d.out, d.wstream, d.ldx, d.ldo = x.data_ptr(), out.data_ptr(), wstream.data_ptr(), x.stride(0), out.stride(0)
    if residual is not None:
        d.residual, d.ldr = _req(residual, torch.float16, "rowlin.residual").data_ptr(), residual.stride(0)
    d.M, d.N, d.K, d.layernorm, d.eps = M, N, K, int(layernorm), eps
    d.frame_bias, d.rows_per_frame, d.frames = int(frames > 0), rows_per_frame, frames
    if gn_ab is not None:   # GroupNorm of x applied on the fly ((scale, shift) pairs from groupnorm_stats)
        d.gn_ab, d.gn_rows = _req(gn_ab, torch.float32, "rowlin.gn_ab").data_ptr(), gn_rows
    stats = None
    if emit_stats:   # finished (mean, rstd) of the output rows for a following folded-LayerNorm GEMM
        stats = torch.empty((M, 2), device=x.device, dtype=torch.float32)
        d.stats_out, d.stats_eps = stats.data_ptr(), stats_eps
    with _timed("gemm_kernel", 2.0 * M * N * K, ("rowlin", M, N, K, int(layernorm), residual is not None)):
        check(lib.insv2v_rowlin(_byref(d), _stream()), "insv2v_rowlin")
    return (out, stats) if emit_stats else out


def rowlin_plan(M, N, K, *, layernorm=False, residual=False, frames=0, rows_per_frame=0, gn_rows=0, cus=0, **over):
    """What insv2v_rowlin does with this problem (insv2v_rowlin_plan, csrc/rows_plan.h): the filled _lib.RowLinPlan - kernel form, one or
    two token blocks per wave, tiles, grid and rounds, or its refusal in .rc.  The descriptor is contiguous with placeholder aligned
    pointers (the planner looks at null and alignment bits only); gn_rows > 0: the GroupNorm-on-load form; cus = 0: this device's CU
    count; `over` sets further descriptor fields (strides, pointers) for the planner's refusals.  Touches no GPU."""
    lib = _lib.load()
    d, p = RowLinDesc(), _lib.RowLinPlan()
    d.x, d.out, d.wstream, d.ldx, d.ldo = 4096, 8192, 12288, K, N
    if residual:   # (True, or a placeholder address of its own)
        d.residual, d.ldr = 16384 if residual is True else int(residual), N
    d.M, d.N, d.K, d.layernorm, d.eps = M, N, K, int(layernorm), 1e-5
    d.frame_bias, d.rows_per_frame, d.frames = int(frames > 0), rows_per_frame, frames
    if gn_rows > 0:
        d.gn_ab, d.gn_rows = 20480, gn_rows
    for key, val in over.items():
        setattr(d, key, val)
    check(lib.insv2v_rowlin_plan(_byref(d), cus, _byref(p)), "insv2v_rowlin_plan")
    return p


def tattn_fused_supported(C, heads, frames):
    """True if insv2v_tattn_fused handles this temporal attention block (C = 320, 8 heads, a window of 1 .. 32 frames)."""
    return int(_lib.load().insv2v_tattn_stream_elems(C, heads, frames)) > 0


def tattn_fused(x, wstream, samples, HW, heads, frames, eps=1e-5, out=None):
    """out = x + to_out(attention over the frames(LayerNorm(x) + pe -> q, k, v)) in one launch (insv2v_tattn_fused); x rows ordered
    (sample, frame, pixel); wstream from fused.pack_tattn_stream with a table of `frames` rows."""
    lib = _lib.load()
    _req(x, torch.float16, "tattn.x"), _req(wstream, torch.float16, "tattn.wstream")
    M, C = x.shape
    if M != samples * frames * HW:
        raise _lib.HipKernelError(f"tattn_fused: {M} rows != {samples} samples x {frames} frames x {HW} pixels")
    if wstream.numel() != int(lib.insv2v_tattn_stream_elems(C, heads, frames)):
        raise _lib.HipKernelError(f"tattn_fused: weight stream of {wstream.numel()} halfs does not match C={C}, heads={heads}, frames={frames}")
    if out is None:
        out = torch.empty((M, C), device=x.device, dtype=torch.float16)
    d = TattnDesc()
    d.x, d.out, d.wstream, d.ldx, d.ldo = x.data_ptr(), out.data_ptr(), wstream.data_ptr(), x.stride(0), out.stride(0)
    d.samples, d.HW, d.C, d.heads, d.frames, d.eps, d.scale = samples, HW, C, heads, frames, eps, (C // heads) ** -0.5
    with _timed("gemm_kernel", 2.0 * M * C * 4 * C + 4.0 * M * frames * C, ("tattn", M, C, heads, frames)):
        check(lib.insv2v_tattn_fused(_byref(d), _stream()), "insv2v_tattn_fused")
    return out


def tattn_attn_supported(C, heads, frames):
    """True if insv2v_tattn_attn handles this temporal attention block (C = 640, 8 heads, a window of 1 .. 32 frames)."""
    return int(_lib.load().insv2v_tattn_attn_stream_elems(C, heads, frames)) > 0


def tattn_attn(x, wstream, samples, HW, heads, frames, eps=1e-5, out=None):
    """out = attention over the frames(LayerNorm(x) + pe -> q, k, v), WITHOUT to_out / residual, in one launch (insv2v_tattn_attn, C = 640);
    x rows ordered (sample, frame, pixel); wstream from fused.pack_tattn_qkv_stream with a table of `frames` rows."""
    lib = _lib.load()
    _req(x, torch.float16, "tattn_attn.x"), _req(wstream, torch.float16, "tattn_attn.wstream")
    M, C = x.shape
    if M != samples * frames * HW:
        raise _lib.HipKernelError(f"tattn_attn: {M} rows != {samples} samples x {frames} frames x {HW} pixels")
    if wstream.numel() != int(lib.insv2v_tattn_attn_stream_elems(C, heads, frames)):
        raise _lib.HipKernelError(f"tattn_attn: weight stream of {wstream.numel()} halfs does not match C={C}, heads={heads}, frames={frames}")
    if out is None:
        out = torch.empty((M, C), device=x.device, dtype=torch.float16)
    d = TattnDesc()
    d.x, d.out, d.wstream, d.ldx, d.ldo = x.data_ptr(), out.data_ptr(), wstream.data_ptr(), x.stride(0), out.stride(0)
    d.samples, d.HW, d.C, d.heads, d.frames, d.eps, d.scale = samples, HW, C, heads, frames, eps, (C // heads) ** -0.5
    with _timed("gemm_kernel", 2.0 * M * C * 3 * C + 4.0 * M * frames * C, ("tattn_attn", M, C, heads, frames)):
        check(lib.insv2v_tattn_attn(_byref(d), _stream()), "insv2v_tattn_attn")
    return out


def xattn_fused_supported(C, heads, ctx_len, rows_per_sample):
    """True if insv2v_xattn_fused handles this text cross-attention block (C = 320, 8 heads, 64 < ctx_len <= 96; every rows_per_sample:
    a sample's rows go in 128-row tiles of its own, fused.row_units)."""
    return int(_lib.load().insv2v_xattn_stream_elems(C, heads, 0)) > 0 and 64 < ctx_len <= 96 and rows_per_sample > 0


def xattn_fused(x, wstream, kvstream, rows_per_sample, heads, ctx_len, eps=1e-5, out=None, pre_residual=None):
    """out = x + to_out(attention(LayerNorm(x) -> q; text K, V of the row's sample)) in one launch (insv2v_xattn_fused).
    wstream from fused.pack_xattn_stream, kvstream [samples, ...] from fused.pack_xattn_kv.
    pre_residual: x is the SELF-attention output and wstream (pack_xattn_stream(pre=...)) starts with that attention's output projection:
    x1 = to_out1(x) + pre_residual replaces x above and never exists in memory."""
    lib = _lib.load()
    _req(x, torch.float16, "xattn.x"), _req(wstream, torch.float16, "xattn.wstream"), _req(kvstream, torch.float16, "xattn.kvstream")
    M, C = x.shape
    if M % rows_per_sample or kvstream.shape[0] != M // rows_per_sample:
        raise _lib.HipKernelError(f"xattn_fused: {M} rows, {rows_per_sample} per sample, K/V streams of {kvstream.shape[0]} samples")
    if wstream.numel() != int(lib.insv2v_xattn_stream_elems(C, heads, 2 if pre_residual is not None else 0)) or \
            kvstream[0].numel() != int(lib.insv2v_xattn_stream_elems(C, heads, 1)):
        raise _lib.HipKernelError(f"xattn_fused: weight / K-V streams do not match C={C}, heads={heads}")
    if out is None:
        out = torch.empty((M, C), device=x.device, dtype=torch.float16)
    d = XattnDesc()
    d.x, d.out, d.wstream, d.kvstream, d.ldx, d.ldo = x.data_ptr(), out.data_ptr(), wstream.data_ptr(), kvstream.data_ptr(), x.stride(0), out.stride(0)
    d.M, d.rows_per_sample, d.C, d.heads, d.ctx_len, d.eps, d.scale = M, rows_per_sample, C, heads, ctx_len, eps, (C // heads) ** -0.5
    if pre_residual is not None:
        d.pre_residual, d.ld_pre = _req(pre_residual, torch.float16, "xattn.pre_residual").data_ptr(), pre_residual.stride(0)
    with _timed("gemm_kernel", (6.0 if pre_residual is not None else 4.0) * M * C * C + 4.0 * M * ctx_len * C, ("xattn", M, C, heads, ctx_len, pre_residual is not None)):
        check(lib.insv2v_xattn_fused(_byref(d), _stream()), "insv2v_xattn_fused")
    return out


def xattn_attn_supported(C, heads, ctx_len, rows_per_sample):
    """True if insv2v_xattn_attn handles this text cross-attention (C = 640, 8 heads, 64 < ctx_len <= 96; every rows_per_sample:
    a sample's rows go in 128-row tiles of its own, fused.row_units)."""
    return int(_lib.load().insv2v_xattn_attn_stream_elems(C, heads, 0)) > 0 and 64 < ctx_len <= 96 and rows_per_sample > 0


def xattn_attn(x, wstream, kvstream, rows_per_sample, heads, ctx_len, eps=1e-5, out=None):
    """out = attention(LayerNorm(x) -> q; text K, V of the row's sample), WITHOUT to_out / residual, in one launch (insv2v_xattn_attn, C = 640).
    wstream from fused.pack_xattn_q_stream, kvstream [samples, ...] from fused.pack_xattn640_kv."""
    lib = _lib.load()
    _req(x, torch.float16, "xattn_attn.x"), _req(wstream, torch.float16, "xattn_attn.wstream"), _req(kvstream, torch.float16, "xattn_attn.kvstream")
    M, C = x.shape
    if M % rows_per_sample or kvstream.shape[0] != M // rows_per_sample:
        raise _lib.HipKernelError(f"xattn_attn: {M} rows, {rows_per_sample} per sample, K/V streams of {kvstream.shape[0]} samples")
    if wstream.numel() != int(lib.insv2v_xattn_attn_stream_elems(C, heads, 0)) or kvstream[0].numel() != int(lib.insv2v_xattn_attn_stream_elems(C, heads, 1)):
        raise _lib.HipKernelError(f"xattn_attn: weight / K-V streams do not match C={C}, heads={heads}")
    if out is None:
        out = torch.empty((M, C), device=x.device, dtype=torch.float16)
    d = XattnDesc()
    d.x, d.out, d.wstream, d.kvstream, d.ldx, d.ldo = x.data_ptr(), out.data_ptr(), wstream.data_ptr(), kvstream.data_ptr(), x.stride(0), out.stride(0)
    d.M, d.rows_per_sample, d.C, d.heads, d.ctx_len, d.eps, d.scale = M, rows_per_sample, C, heads, ctx_len, eps, (C // heads) ** -0.5
    with _timed("gemm_kernel", 2.0 * M * C * C + 4.0 * M * ctx_len * C, ("xattn_attn", M, C, heads, ctx_len)):
        check(lib.insv2v_xattn_attn(_byref(d), _stream()), "insv2v_xattn_attn")
    return out


def _conv_geometry(geom, stride, pad, upsample, out_size=None):
    NB, IH, IW = geom
    if out_size is not None:   # nearest-x2 upsample to an explicit size: the library checks OH in {2 IH - 1, 2 IH} (and OW alike)
        if not upsample:
            raise ValueError("conv3x3: out_size is the target of the nearest-x2 upsample (upsample=True)")
        return int(out_size[0]), int(out_size[1])
    IHu, IWu = (IH * 2, IW * 2) if upsample else (IH, IW)
    pt, pl = pad
    # PyTorch conv arithmetic; the VAE's asymmetric (0,1,0,1) pad is pad=(0,0) with one extra row/col
    if pt == 0 and stride == 2:
        return (IHu + 1 - 3) // 2 + 1, (IWu + 1 - 3) // 2 + 1
    return (IHu + 2 * pt - 3) // stride + 1, (IWu + 2 * pl - 3) // stride + 1


_FUSE_CACHE = {}


class operand_window:
    """Context manager for tests: insv2v_gemm and the launchers of the fused row kernels (ffn_fused, tattn_*, xattn_*) treat ``nbytes`` as
    the size of one operand window, so a small problem takes the path of an operand beyond 2 GiB (row / image / tile / sample ranges, one
    launch each).  The product never uses it."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)

    def __enter__(self):
        self.prev = int(_lib.load().insv2v_set_operand_window(self.nbytes))
        _STATS_PARTS_CACHE.clear()   # insv2v_gemm_stats_parts answers for the window in force (a split problem emits none)

    def __exit__(self, *exc):
        _lib.load().insv2v_set_operand_window(self.prev)
        _STATS_PARTS_CACHE.clear()
        return False


def tap_weights(w):
    """[Cout <= 4, Cin, 3, 3] convolution weights -> the [40, Cin] fp16 matrix of conv3x3_narrow: row 4 t + c = w[c, :, ky, kx], t = 3 ky + kx
    (rows of absent output channels and rows 36-39 are zero)."""
    cout, cin = w.shape[:2]
    if cout > 4 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"tap_weights: a 3x3 convolution with <= 4 output channels, got {tuple(w.shape)}")
    wt = torch.zeros(40, cin, dtype=torch.float32)
    wt[:36].reshape(9, 4, cin)[:, :cout] = w.detach().float().cpu().permute(2, 3, 0, 1).reshape(9, cout, cin)
    return wt.half()


def conv3x3_narrow(x, geom, wtap, bias, cout):
    """Stride-1, pad-1 3x3 convolution with <= 4 output channels as ONE plain GEMM over the input channels (the nine taps' partial outputs
    of every pixel, fp32) + insv2v_tap_gather (the shifted sum): x [NB*H*W, Cin] fp16, wtap = tap_weights(w) on the device -> fp32 [NB*H*W, cout].
    The direct implicit-GEMM form pads the output channels to a 64-wide tile: 16 x the multiply-adds at cout = 4."""
    lib = _lib.load()
    NB, H, W = geom
    y9 = gemm(x, wtap, None, out_fp32=True)
    out = torch.empty((x.shape[0], cout), device=x.device, dtype=torch.float32)
    with _timed("elementwise", 0.0, ("tapgather", x.shape[0], cout)):
        check(lib.insv2v_tap_gather(y9.data_ptr(), y9.stride(0), _ptr(bias), out.data_ptr(), out.stride(0), NB, H, W, cout, _stream()), "insv2v_tap_gather")
    return out


def conv3x3_fuses_groupnorm(geom, cin, cout, k_split=0):
    """True if a stride-1, pad-1 3x3 convolution of this geometry runs on the patch-tiled kernel, which can apply the
    preceding GroupNorm(+SiLU) to its input patch in LDS (conv3x3(gn_ab=...)); asked of the library, cached."""
    key = (tuple(geom), cin, cout, k_split)
    if key not in _FUSE_CACHE:
        lib = _lib.load()
        NB, IH, IW = geom
        d = GemmDesc()
        d.M, d.N, d.K, d.batch, d.mode = NB * IH * IW, cout, 9 * cin, 1, 1
        d.NB, d.IH, d.IW, d.OH, d.OW, d.Cin = NB, IH, IW, IH, IW, cin
        d.stride, d.pad_t, d.pad_l, d.k_split = 1, 1, 1, k_split
        d.workspace, d.workspace_bytes = 1, WORKSPACE_BYTES  # only the decision logic looks at these
        _FUSE_CACHE[key] = bool(lib.insv2v_conv3x3_fuses_groupnorm(_byref(d)))
    return _FUSE_CACHE[key]


def conv3x3(x, geom, w, bias=None, *, x2=None, stride=1, pad=(1, 1), upsample=False, residual=None, row_bias=None,
            rows_per_group=0, out_fp32=False, tile=0, split_k=0, gn_ab=None, gn_images_per_sample=0, gn_silu=False, out=None, act=ACT_NONE,
            out_size=None):
    """3x3 convolution over channels-last pixels.  x: [NB*IH*IW, C1] (+x2 [.., C2]); w: [N, 9*(C1+C2)];
    geom = (NB, IH, IW).  Returns ([NB*OH*OW, N], (NB, OH, OW)).
    out_size = (OH, OW) with upsample=True: the nearest-x2 image is taken WITHOUT its last row where OH = 2 IH - 1 (column: OW = 2 IW - 1) -
    F.interpolate(size=out_size, mode="nearest"), Upsample3D's output_size - and zero-padded at that edge; None: exactly x2.
    gn_ab ([nsamples, C1+C2, 2] fp32 from groupnorm_stats): x is the RAW tensor and the kernel applies
    act(x*scale + shift) to its input on the fly (only where conv3x3_fuses_groupnorm says so).
    An input beyond the 2 GiB descriptor window of the kernels' LDS-DMA loads (the normalised [1 474 560, 960] concatenation entering
    the first level-0 up block at 20 stacked clips) is convolved by insv2v_gemm in image-aligned parts, one launch each (round 5: the
    split lives behind the C ABI, for the Linear form too)."""
    lib = _lib.load()
    _req(x, torch.float16, "conv.x"), _req(w, torch.float16, "conv.w")
    NB, IH, IW = geom
    pt, pl = pad
    OH, OW = _conv_geometry(geom, stride, pad, upsample, out_size)
    N = w.shape[0]
    cin = x.shape[1] + (x2.shape[1] if x2 is not None else 0)
    M = NB * OH * OW
    if out is None:
        out = torch.empty((M, N), device=x.device, dtype=torch.float32 if out_fp32 else torch.float16)
    d = GemmDesc()
    d.a, d.w, d.c = x.data_ptr(), w.data_ptr(), out.data_ptr()
    d.lda, d.ldw, d.ldc = x.stride(0), w.stride(0), out.stride(0)
    if x2 is not None:
        d.a2, d.lda2, d.k_split = _req(x2, torch.float16, "conv.x2").data_ptr(), x2.stride(0), x.shape[1]
    if bias is not None:
        d.bias = _req(bias, torch.float32, "conv.bias").data_ptr()
    if row_bias is not None:
        d.row_bias, d.ld_rb, d.rows_per_group = _req(row_bias, torch.float32, "conv.row_bias").data_ptr(), row_bias.stride(0), rows_per_group
    if residual is not None:
        d.residual, d.ldr = _req(residual, torch.float16, "conv.residual").data_ptr(), residual.stride(0)
    d.M, d.N, d.K, d.c_fp32, d.alpha, d.tile, d.batch, d.act = M, N, 9 * cin, int(out_fp32), 1.0, tile, 1, act
    d.mode, d.NB, d.IH, d.IW, d.OH, d.OW, d.Cin = 1, NB, IH, IW, OH, OW, cin
    d.stride, d.pad_t, d.pad_l, d.upsample = stride, pt, pl, int(upsample)
    if gn_ab is not None:
        d.gn_ab = _req(gn_ab, torch.float32, "conv.gn_ab").data_ptr()
        d.gn_images_per_sample, d.gn_silu = gn_images_per_sample, int(gn_silu)
    ws = _workspace(x.device)
    d.workspace, d.workspace_bytes, d.split_k = ws.data_ptr(), ws.numel() * 4, split_k
    with _timed("gemm_kernel", 2.0 * M * N * 9 * cin, ("conv", M, N, 9 * cin, stride, int(upsample), residual is not None)):
        check(lib.insv2v_gemm(_byref(d), _stream()), "insv2v_gemm(conv3x3)")
    return out, (NB, OH, OW)


def _gn_chunks(nsamples, rows_per_sample):
    """Chunks per sample of the GroupNorm statistics pass.  (More, smaller chunks - up to 512 per sample - were A/B-ed in round 2
    and lost 0.2 ms per UNet step to the longer finalize; the pass itself now keeps four 16-byte loads per thread in flight.)"""
    return max(1, min(rows_per_sample // 32, max(1, 1024 // nsamples), 128))


# ---- Winograd F(2x2, 3x3) convolution (insv2v_winograd_input -> grouped insv2v_gemm -> insv2v_winograd_output; csrc/winograd.hip)
_WINO_G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])


def winograd_weights(w, device, upsample=False):
    """[Cout, Cin, 3, 3] fp32 convolution weights -> U [16, Cout, Cin] fp16, U[i*4 + j] = (G g G^T)[i][j] (computed in fp32, rounded once).
    upsample: the 9 matrices of the nearest-x2-upsample form, patch indices (i, j) in {0, 1, 3}^2 (the others meet an all-zero V)."""
    u = torch.einsum("ai,ocij,bj->aboc", _WINO_G, w.float(), _WINO_G)   # [4, 4, Cout, Cin]
    if upsample:
        u = u[[0, 1, 3]][:, [0, 1, 3]]
    return u.reshape(-1, w.shape[0], w.shape[1]).to(device=device, dtype=torch.float16).contiguous()


def winograd_ok(geom, cin, c1=0, upsample=False, out_size=None):
    """Shapes insv2v_winograd_input accepts (else the caller uses conv3x3): any H, W (odd sizes: the last tile row / column hangs over the
    image, reads zeros there and stores only the pixels that exist); image rows of at most 128 pixels (an image's 64-channel slice is staged
    in LDS whole or in bands of tile rows).  upsample: one tile per input pixel, exact x2 only - the 9-tap form rests on the patch's two
    centre rows / columns being equal, which a cropped target (out_size != (2 H, 2 W)) breaks at its zero-padded edge."""
    _, H, W = geom
    if upsample and out_size is not None and tuple(out_size) != (2 * H, 2 * W):
        return False
    return W <= 128 and cin % 64 == 0 and c1 % 64 == 0


def winograd_conv3x3(x, geom, U, bias=None, *, x2=None, gn_ab=None, gn_images_per_sample=0, gn_silu=False, row_bias=None, rows_per_group=0,
                     residual=None, out=None, tile=0, upsample=False):
    """Stride-1, pad-1 3x3 convolution over channels-last pixels in Winograd form: x [NB*H*W, C1] (+ x2 [.., C2]), U = winograd_weights(w)
    [16, Cout, C1 + C2]; optional GroupNorm (+SiLU) of the input from the (scale, shift) table gn_ab (groupnorm_stats).  Returns [NB*H*W, Cout]."""
    lib = _lib.load()
    _req(x, torch.float16, "winograd.x"), _req(U, torch.float16, "winograd.U")
    NB, H, W = geom
    C1 = x.shape[1]
    C = C1 + (x2.shape[1] if x2 is not None else 0)
    Cout = U.shape[1]
    ng = 9 if upsample else 16                     # transformed taps that are not identically zero
    OH, OW = (2 * H, 2 * W) if upsample else (H, W)
    assert U.shape[0] == ng and U.shape[2] == C and x.shape[0] == NB * H * W
    tiles = NB * H * W if upsample else NB * ((H + 1) // 2) * ((W + 1) // 2)   # odd H / W: the last tile row / column is half outside
    grows = -(-tiles // 256) * 256
    v = torch.empty((ng * grows, C), device=x.device, dtype=torch.float16)
    di = WinogradInDesc()
    di.x, di.v, di.ldx, di.v_group_rows = x.data_ptr(), v.data_ptr(), x.stride(0), grows
    if x2 is not None:
        di.x2, di.ldx2, di.C1 = _req(x2, torch.float16, "winograd.x2").data_ptr(), x2.stride(0), C1
    di.NB, di.H, di.W, di.C, di.upsample = NB, H, W, C, int(upsample)
    if gn_ab is not None:
        di.gn_ab, di.gn_images_per_sample, di.gn_silu = _req(gn_ab, torch.float32, "winograd.gn_ab").data_ptr(), gn_images_per_sample, int(gn_silu)
    with _timed("groupnorm", 0.0, ("wino_in", NB * H * W, C)):
        check(lib.insv2v_winograd_input(_byref(di), _stream()), "insv2v_winograd_input")
    m = torch.empty((ng * grows, Cout), device=x.device, dtype=torch.float16)
    d = GemmDesc()
    d.a, d.w, d.c = v.data_ptr(), U.data_ptr(), m.data_ptr()
    d.lda, d.ldw, d.ldc = C, C, Cout
    d.M, d.N, d.K, d.batch, d.alpha, d.tile = ng * grows, Cout, C, 1, 1.0, tile
    d.w_group_rows, d.w_group_stride = grows, Cout * C
    # (recorded work = the ALGORITHMIC work of the convolution, 2 * pixels * Cout * 9 * C as SURVEY.md 8d counts it; the launch performs
    #  4 / 9 of those multiply-adds - the tag carries the launched product's shape)
    with _timed("gemm_kernel", 2.0 * NB * OH * OW * Cout * 9 * C, ("wino_gemm", ng * grows, Cout, C)):
        check(lib.insv2v_gemm(_byref(d), _stream()), "insv2v_gemm (grouped)")
    del v
    if out is None:
        out = torch.empty((NB * OH * OW, Cout), device=x.device, dtype=torch.float16)
    do = WinogradOutDesc()
    do.m, do.y, do.m_group_rows, do.ldy = m.data_ptr(), out.data_ptr(), grows, out.stride(0)
    if bias is not None:
        do.bias = _req(bias, torch.float32, "winograd.bias").data_ptr()
    if row_bias is not None:
        do.row_bias, do.ld_rb, do.rows_per_group = _req(row_bias, torch.float32, "winograd.row_bias").data_ptr(), row_bias.stride(0), rows_per_group
    if residual is not None:
        do.residual, do.ldr = _req(residual, torch.float16, "winograd.residual").data_ptr(), residual.stride(0)
    do.NB, do.H, do.W, do.Cout, do.upsample = NB, H, W, Cout, int(upsample)
    with _timed("groupnorm", 0.0, ("wino_out", NB * OH * OW, Cout)):
        check(lib.insv2v_winograd_output(_byref(do), _stream()), "insv2v_winograd_output")
    return out


def groupnorm(x, nsamples, rows_per_sample, gamma, beta, groups, eps, silu=False, x2=None):
    """GroupNorm(+SiLU) of channels-last tokens; nsamples*rows_per_sample == x.shape[0].
    (Normalising in groups of samples so that the apply pass re-reads what the statistics pass just streamed was measured and is
    slower: profiles/r04_groupnorm_sample_groups_experiment.txt.)"""
    lib = _lib.load()
    _req(x, torch.float16, "groupnorm.x")
    C1 = x.shape[1]
    Ct = C1 + (x2.shape[1] if x2 is not None else 0)
    assert nsamples * rows_per_sample == x.shape[0]
    y = torch.empty((x.shape[0], Ct), device=x.device, dtype=torch.float16)
    nchunks = _gn_chunks(nsamples, rows_per_sample)
    # stats [nsamples,G,2] + partials [nsamples,nchunks,G,3]; allocated per call so graph capture owns it
    scratch = torch.empty(nsamples * groups * (2 + 3 * nchunks), device=x.device, dtype=torch.float32)
    d = GroupNormDesc()
    d.x, d.y, d.gamma, d.beta, d.partials = x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr(), scratch.data_ptr()
    d.ldx, d.ldy = x.stride(0), y.stride(0)
    if x2 is not None:
        d.x2, d.ldx2, d.C1 = _req(x2, torch.float16, "groupnorm.x2").data_ptr(), x2.stride(0), C1
    d.nsamples, d.rows_per_sample, d.C, d.G, d.nchunks, d.silu, d.eps = nsamples, rows_per_sample, Ct, groups, nchunks, int(silu), eps
    with _timed("groupnorm", 0.0, ("gn", nsamples, rows_per_sample, Ct)):
        check(lib.insv2v_groupnorm(_byref(d), _stream()), "insv2v_groupnorm")
    return y


def groupnorm_stats(x, nsamples, rows_per_sample, gamma, beta, groups, eps, x2=None):
    """GroupNorm statistics only -> ab [nsamples, C, 2] fp32 = (rstd*gamma, beta - mean*rstd*gamma) per channel, for a
    consumer that normalises on the fly (conv3x3(gn_ab=...)): one read of the tensor, no normalised copy."""
    lib = _lib.load()
    _req(x, torch.float16, "groupnorm.x")
    C1 = x.shape[1]
    Ct = C1 + (x2.shape[1] if x2 is not None else 0)
    assert nsamples * rows_per_sample == x.shape[0]
    nchunks = _gn_chunks(nsamples, rows_per_sample)
    scratch = torch.empty(nsamples * groups * (2 + 3 * nchunks), device=x.device, dtype=torch.float32)
    ab = torch.empty((nsamples, Ct, 2), device=x.device, dtype=torch.float32)
    d = GroupNormDesc()
    d.x, d.gamma, d.beta, d.partials, d.ab = x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), scratch.data_ptr(), ab.data_ptr()
    d.ldx, d.stats_only = x.stride(0), 1
    if x2 is not None:
        d.x2, d.ldx2, d.C1 = _req(x2, torch.float16, "groupnorm.x2").data_ptr(), x2.stride(0), C1
    d.nsamples, d.rows_per_sample, d.C, d.G, d.nchunks, d.eps = nsamples, rows_per_sample, Ct, groups, nchunks, eps
    with _timed("groupnorm", 0.0, ("gnstats", nsamples, rows_per_sample, Ct)):
        check(lib.insv2v_groupnorm(_byref(d), _stream()), "insv2v_groupnorm(stats_only)")
    return ab


def layernorm(x, gamma, beta, eps=1e-5, pe=None, rows_per_frame=0, frames=0, pe_start=0):
    lib = _lib.load()
    _req(x, torch.float16, "layernorm.x")
    y = torch.empty_like(x)
    d = LayerNormDesc()
    d.x, d.y, d.gamma, d.beta = x.data_ptr(), y.data_ptr(), gamma.data_ptr(), beta.data_ptr()
    d.ldx, d.ldy, d.rows, d.C, d.eps = x.stride(0), y.stride(0), x.shape[0], x.shape[1], eps
    if pe is not None:
        d.pe, d.rows_per_frame, d.frames, d.pe_start = _req(pe, torch.float32, "layernorm.pe").data_ptr(), rows_per_frame, frames, pe_start
    with _timed("layernorm", 0.0, ("ln", x.shape[0], x.shape[1])):
        check(lib.insv2v_layernorm(_byref(d), _stream()), "insv2v_layernorm")
    return y


def layernorm_stats(x, eps=1e-5):
    """(mean, rstd) per token row -> fp32 [rows, 2]; consumed by gemm(row_stats=...)."""
    lib = _lib.load()
    _req(x, torch.float16, "layernorm_stats.x")
    stats = torch.empty((x.shape[0], 2), device=x.device, dtype=torch.float32)
    with _timed("layernorm", 0.0, ("lnstats", x.shape[0], x.shape[1])):
        check(lib.insv2v_layernorm_stats(x.data_ptr(), stats.data_ptr(), x.stride(0), x.shape[0], x.shape[1], eps, _stream()),
              "insv2v_layernorm_stats")
    return stats


def attention(q_ptr, k_ptr, v_ptr, out, *, batch, heads, head_dim, seq_q, seq_k, scale,
              q_rs, k_rs, v_rs, o_rs, q_addr, kv_addr, o_addr, causal=False, qkv_bias=None):
    """*_addr = (inner, outer_stride, step): base offset of problem z = (z//inner)*outer + (z%inner)*step.
    qkv_bias: fp16 table [seq, 3 * heads * head_dim] added to the q | k | v rows of sequence position i as they are loaded (the temporal
    positional encoding pushed through the projections); only the <= 16-row form (attention_short_supported) takes it."""
    lib = _lib.load()
    d = AttentionDesc()
    if qkv_bias is not None:
        _req(qkv_bias, torch.float16, "attention.qkv_bias")
        cq = heads * head_dim
        if qkv_bias.shape[0] < max(seq_q, seq_k) or qkv_bias.shape[1] != 3 * cq:
            raise _lib.HipKernelError(f"attention: bias table {tuple(qkv_bias.shape)} for {max(seq_q, seq_k)} rows x 3 x {cq} columns")
        bp = qkv_bias.data_ptr()
        d.q_bias, d.k_bias, d.v_bias, d.bias_rs = bp, bp + 2 * cq, bp + 4 * cq, qkv_bias.stride(0)
    d.q, d.k, d.v, d.o = q_ptr, k_ptr, v_ptr, out.data_ptr()
    d.q_rs, d.k_rs, d.v_rs, d.o_rs = q_rs, k_rs, v_rs, o_rs
    d.q_inner, d.q_outer, d.q_step = q_addr
    d.kv_inner, d.kv_outer, d.kv_step = kv_addr
    d.o_inner, d.o_outer, d.o_step = o_addr
    d.batch, d.heads, d.head_dim, d.seq_q, d.seq_k, d.scale, d.causal = batch, heads, head_dim, seq_q, seq_k, scale, int(causal)
    with _timed("attn_kernel", 4.0 * batch * heads * seq_q * seq_k * head_dim, ("attn", batch, heads, head_dim, seq_q, seq_k)):
        check(lib.insv2v_attention(_byref(d), _stream()), "insv2v_attention")
    return out


def attention_short_supported(heads, head_dim, seq, biased=False):
    """True if insv2v_attention runs the one-wave-per-head kernel for a temporal self-attention of `seq` frames (the only kernel that takes
    qkv_bias); biased=True: with the bias tables.  The library's planner answers (insv2v_attention_plan): no rule is restated here."""
    lib = _lib.load()
    d, p = AttentionDesc(), _lib.AttentionPlan()
    d.q = d.k = d.v = d.o = 16          # (the planner looks at null and alignment bits only)
    if biased:
        d.q_bias = d.k_bias = d.v_bias = 16
        d.bias_rs = 3 * heads * head_dim
    d.q_rs = d.k_rs = d.v_rs = 3 * heads * head_dim
    d.o_rs = heads * head_dim
    d.q_inner = d.kv_inner = d.o_inner = 1
    d.batch, d.heads, d.head_dim, d.seq_q, d.seq_k, d.scale = 1, heads, head_dim, seq, seq, 1.0
    check(lib.insv2v_attention_plan(_byref(d), 0, _byref(p)), "insv2v_attention_plan")
    return p.rc == 0 and p.family in (_lib.ATTN_PLAN_SHORT, _lib.ATTN_PLAN_SHORT_BIAS)


def embed_tokens(ids, tok, pos):
    """CLIP text embeddings: ids int64 [n, L] (device) -> fp16 [n*L, C] = tok[ids] + pos[position]."""
    lib = _lib.load()
    _req(tok, torch.float16, "embed.tok")
    _req(pos, torch.float16, "embed.pos")
    if ids.dtype != torch.int64 or not ids.is_cuda or not ids.is_contiguous():
        raise _lib.HipKernelError("embed.ids must be a contiguous int64 device tensor")
    n, L = ids.shape
    if L > pos.shape[0]:
        raise ValueError(f"Sequence length must be less than max_position_embeddings (got {L} > {pos.shape[0]})")
    out = torch.empty((n * L, tok.shape[1]), device=tok.device, dtype=torch.float16)
    check(lib.insv2v_embed_tokens(ids.data_ptr(), tok.data_ptr(), pos.data_ptr(), out.data_ptr(), n * L, L, tok.shape[1],
                                  tok.shape[0], _stream()), "insv2v_embed_tokens")
    return out


def softmax_rows(x, scale=1.0, valid=None):
    """In-place row softmax of the last dimension; valid < x.shape[-1]: over the first `valid` columns, the others become exact zeros."""
    lib = _lib.load()
    _req(x, torch.float16, "softmax.x")
    x2 = x.reshape(-1, x.shape[-1])
    if valid is not None and valid != x2.shape[1]:
        check(lib.insv2v_softmax_rows_padded(x2.data_ptr(), x2.data_ptr(), x2.stride(0), x2.stride(0), x2.shape[0], x2.shape[1], valid,
                                             scale, _stream()), "insv2v_softmax_rows_padded")
        return x
    check(lib.insv2v_softmax_rows(x2.data_ptr(), x2.data_ptr(), x2.stride(0), x2.stride(0), x2.shape[0], x2.shape[1],
                                  scale, _stream()), "insv2v_softmax_rows")
    return x


def timestep_embedding(t_dev, dim, shift=0.0):
    lib = _lib.load()
    _req(t_dev, torch.float32, "timestep")
    out = torch.empty((t_dev.shape[0], dim), device=t_dev.device, dtype=torch.float16)
    check(lib.insv2v_timestep_embedding(t_dev.data_ptr(), out.data_ptr(), t_dev.shape[0], dim, shift, _stream()),
          "insv2v_timestep_embedding")
    return out


def build_unet_input(latent, img_cond, out, t_out, timestep, nbranch, branch_rows=0, t_stride=0):
    """branch_rows / t_stride: rows of ``out`` / entries of ``t_out`` between consecutive branches (0: back to back) - the branch-major
    layout of a stack of clips (inference._stacked_gen)."""
    lib = _lib.load()
    F, _, h, w = latent.shape[-4:]
    check(lib.insv2v_build_unet_input(_req(latent, torch.float32, "latent").data_ptr(),
                                      _req(img_cond, torch.float32, "img_cond").data_ptr(), out.data_ptr(),
                                      _ptr(t_out), float(timestep), nbranch, F, h, w, out.shape[-1], branch_rows, t_stride, _stream()),
          "insv2v_build_unet_input")
    return out


def cfg_step(eps_in, latent, *, nbranch, text_cfg=1.0, img_cfg=1.0, sqrt_a=1.0, sqrt_1ma=0.0, coef=(0, 0, 0, 0),
             latent_out=None, pred_x0=None, eps_out=None, latent_ref=None, correct=0, delta_q=None, noise=None,
             rescale_stats=None, guidance_rescale=0.0, branch_stride=0, noise_seed=None, noise_stream=0, x0_hist=None, c_hist=0.0,
             mask=None, src=None, known_noise=None, k_src=0.0, k_noise=0.0, release=None, step=0):
    """``noise_seed`` / ``noise_stream``: the step's variance noise is generated inside the kernel from the seeded stream (element = flat
    index of [F,4,h,w]) instead of read from ``noise``; passing both is rejected by the kernel.
    ``x0_hist`` / ``c_hist``: the multistep term ``c_hist * x0_hist`` (the previous step's ``pred_x0``, DPM-Solver++ 2M).  Only a call
    that gives a history goes to insv2v_cfg_step_ms (``cfg_step_ms``); every other call goes to insv2v_cfg_step as before.
    ``mask`` [F,h,w] with ``src`` / ``known_noise`` [F,4,h,w] and ``k_src`` / ``k_noise``: behind the update, ``latent_out`` becomes
    ``mask * prev + (1 - mask) * (k_src * src + k_noise * known_noise)`` (insv2v_cfg_step_mask, ``cfg_step_mask``).  Only a call that
    gives a mask goes there.
    ``release`` int32 [F,h,w] with ``step``, the step's GLOBAL index: a cell is held like one outside the mask until
    ``release <= step`` (insv2v_cfg_step_release, ``cfg_step_release``; ``mask`` may then be None = 1).  Only a call that gives a
    release map goes there."""
    kw = dict(nbranch=nbranch, text_cfg=text_cfg, img_cfg=img_cfg, sqrt_a=sqrt_a, sqrt_1ma=sqrt_1ma, coef=coef, latent_out=latent_out,
              pred_x0=pred_x0, eps_out=eps_out, latent_ref=latent_ref, correct=correct, delta_q=delta_q, noise=noise,
              rescale_stats=rescale_stats, guidance_rescale=guidance_rescale, branch_stride=branch_stride, noise_seed=noise_seed,
              noise_stream=noise_stream)
    if release is not None:
        return cfg_step_release(eps_in, latent, release=release, step=step, mask=mask, src=src, known_noise=known_noise, k_src=k_src,
                                k_noise=k_noise, x0_hist=x0_hist, c_hist=c_hist, **kw)
    if mask is not None:
        return cfg_step_mask(eps_in, latent, mask=mask, src=src, known_noise=known_noise, k_src=k_src, k_noise=k_noise, x0_hist=x0_hist,
                             c_hist=c_hist, **kw)
    if src is not None or known_noise is not None:
        raise _lib.HipKernelError("cfg_step: src / known_noise need a mask")
    if x0_hist is not None:
        return cfg_step_ms(eps_in, latent, x0_hist=x0_hist, c_hist=c_hist, **kw)
    if c_hist != 0.0:
        raise _lib.HipKernelError("cfg_step: c_hist != 0 needs x0_hist")
    lib = _lib.load()
    d = _fill_step_desc(StepDesc(), eps_in, latent, **kw)
    check(lib.insv2v_cfg_step(_byref(d), _stream()), "insv2v_cfg_step")


def cfg_step_ms(eps_in, latent, *, x0_hist=None, c_hist=0.0, **kw):
    """insv2v_cfg_step_ms: ``cfg_step`` (its keywords) plus ``c_hist * x0_hist`` in the update.  ``x0_hist`` fp32 [F,4,h,w] or None
    (then the result is bit-identical to ``cfg_step``); it must not overlap an output."""
    lib = _lib.load()
    d = _fill_step_desc(MStepDesc(), eps_in, latent, **kw)
    if x0_hist is not None and (tuple(x0_hist.shape[-4:]) != tuple(latent.shape[-4:]) or not x0_hist.is_contiguous()):
        raise _lib.HipKernelError(f"cfg_step_ms: x0_hist {tuple(x0_hist.shape)} must be contiguous and shaped like the latent {tuple(latent.shape)}")
    d.x0_hist = _req(x0_hist, torch.float32, "x0_hist").data_ptr() if x0_hist is not None else None
    d.c_hist = c_hist
    check(lib.insv2v_cfg_step_ms(_byref(d), _stream()), "insv2v_cfg_step_ms")


def cfg_step_mask(eps_in, latent, *, mask=None, src=None, known_noise=None, k_src=0.0, k_noise=0.0, x0_hist=None, c_hist=0.0, **kw):
    """insv2v_cfg_step_mask: ``cfg_step_ms`` (its keywords) plus the blend of ``latent_out`` with the re-noised source latent outside
    ``mask``.  ``mask`` fp32 [F,h,w] or None (then the result is bit-identical to ``cfg_step_ms`` / ``cfg_step``); ``src`` and
    ``known_noise`` fp32 [F,4,h,w]; none of them may overlap an output."""
    lib = _lib.load()
    d = _fill_known_desc(MaskStepDesc(), "cfg_step_mask", eps_in, latent, mask, src, known_noise, k_src, k_noise, x0_hist, c_hist, kw)
    check(lib.insv2v_cfg_step_mask(_byref(d), _stream()), "insv2v_cfg_step_mask")


def cfg_step_release(eps_in, latent, *, release=None, step=0, mask=None, src=None, known_noise=None, k_src=0.0, k_noise=0.0, x0_hist=None,
                     c_hist=0.0, **kw):
    """insv2v_cfg_step_release: ``cfg_step_mask`` (its keywords) with a per-cell gate in front of the blend - ``release`` int32 [F,h,w]
    or None (then the result is bit-identical to ``cfg_step_mask``), ``step`` the step's global index in the scheduler's timesteps: a
    cell with ``release > step`` is held at the re-noised source whatever ``mask`` says; ``mask`` None means 1 everywhere."""
    lib = _lib.load()
    d = _fill_known_desc(RelStepDesc(), "cfg_step_release", eps_in, latent, mask, src, known_noise, k_src, k_noise, x0_hist, c_hist, kw)
    if release is not None:
        want = (latent.shape[-4],) + tuple(latent.shape[-2:])
        _req(release, torch.int32, "release")
        if tuple(release.shape[-3:]) != want or release.numel() != math.prod(want) or not release.is_contiguous():
            raise _lib.HipKernelError(f"cfg_step_release: release {tuple(release.shape)} must be contiguous and shaped {want} (latent {tuple(latent.shape)})")
    if isinstance(step, bool) or not isinstance(step, int) or not -2 ** 31 <= step < 2 ** 31:
        raise _lib.HipKernelError(f"cfg_step_release: step {step!r} must be an int32")
    d.release, d.step = _ptr(release), step
    check(lib.insv2v_cfg_step_release(_byref(d), _stream()), "insv2v_cfg_step_release")


def strength_release(smap, steps, mode="max", mask=None):
    """insv2v_strength_release (tests/strength_map_ref.py is the definition): strength image ``smap`` fp32
    [..., H, W] in [0,1] -> (release int32 [..., H/8, W/8], gate fp32 [..., H, W]).  ``release`` = ``steps`` minus the steps the cell's
    strength (``mask_to_latent(smap, mode)``, bit for bit) executes, ``schedulers.strength_to_start`` per cell; ``gate`` = 0 where
    ``smap`` <= 0 or NaN, elsewhere ``mask`` (an image-resolution mask shaped like ``smap``) or 1."""
    if mode not in ("mean", "max"):
        raise ValueError(f"strength_release: mode {mode!r} is neither 'mean' nor 'max'")
    lib = _lib.load()
    _req(smap, torch.float32, "strength_release.smap")
    if smap.dim() < 2:
        raise _lib.HipKernelError(f"strength_release: smap {tuple(smap.shape)} needs [..., H, W]")
    smap = smap.contiguous()
    if mask is not None:
        _req(mask, torch.float32, "strength_release.mask")
        if mask.shape != smap.shape:
            raise _lib.HipKernelError(f"strength_release: mask {tuple(mask.shape)} must be shaped like smap {tuple(smap.shape)}")
        mask = mask.contiguous()
    H, W = smap.shape[-2:]
    N = smap.numel() // max(H * W, 1)
    release = torch.empty((*smap.shape[:-2], H // 8, W // 8), device=smap.device, dtype=torch.int32)
    gate = torch.empty_like(smap)
    check(lib.insv2v_strength_release(smap.data_ptr(), _ptr(mask), release.data_ptr(), gate.data_ptr(), N, H, W, 1 if mode == "max" else 0,
                                      int(steps), _stream()), "insv2v_strength_release")
    return release, gate


def _fill_known_desc(d, who, eps_in, latent, mask, src, known_noise, k_src, k_noise, x0_hist, c_hist, kw):
    """The step descriptor ``d`` (MaskStepDesc or one that begins with it) of a call with a known region."""
    d = _fill_step_desc(d, eps_in, latent, **kw)
    shape = tuple(latent.shape[-4:])
    for name, t, want in (("x0_hist", x0_hist, shape), ("src", src, shape), ("known_noise", known_noise, shape),
                          ("mask", mask, (shape[0],) + shape[2:])):
        if t is None:
            continue
        _req(t, torch.float32, name)
        if tuple(t.shape[-len(want):]) != want or t.numel() != math.prod(want) or not t.is_contiguous():
            raise _lib.HipKernelError(f"{who}: {name} {tuple(t.shape)} must be contiguous and shaped {want} (latent {tuple(latent.shape)})")
    d.x0_hist, d.c_hist = _ptr(x0_hist), c_hist
    d.mask, d.src, d.known_noise, d.k_src, d.k_noise = _ptr(mask), _ptr(src), _ptr(known_noise), k_src, k_noise
    return d


def mask_to_latent(mask, mode="max"):
    """Image-resolution mask fp32 [..., H, W] -> latent resolution [..., H/8, W/8]: per 8x8 cell its ``mode`` "mean" or "max"."""
    if mode not in ("mean", "max"):
        raise ValueError(f"mask_to_latent: mode {mode!r} is neither 'mean' nor 'max'")
    lib = _lib.load()
    _req(mask, torch.float32, "mask_to_latent.mask")
    if mask.dim() < 2:
        raise _lib.HipKernelError(f"mask_to_latent: mask {tuple(mask.shape)} needs [..., H, W]")
    mask = mask.contiguous()
    H, W = mask.shape[-2:]
    N = mask.numel() // max(H * W, 1)
    out = torch.empty((*mask.shape[:-2], H // 8, W // 8), device=mask.device, dtype=torch.float32)
    check(lib.insv2v_mask_to_latent(mask.data_ptr(), out.data_ptr(), N, H, W, 1 if mode == "max" else 0, _stream()), "insv2v_mask_to_latent")
    return out


def composite(edited, original, mask, out=None):
    """clip(mask * edited + (1 - mask) * original, -1, 1) on fp32 [N,3,H,W] frames with an image-resolution mask [N,H,W]; ``out`` may be
    ``edited``."""
    lib = _lib.load()
    for name, t in (("edited", edited), ("original", original), ("mask", mask)):
        _req(t, torch.float32, "composite." + name)
        if not t.is_contiguous():
            raise _lib.HipKernelError(f"composite: {name} must be contiguous")
    if edited.dim() != 4 or edited.shape[1] != 3 or original.shape != edited.shape or tuple(mask.shape) != (edited.shape[0], *edited.shape[2:]):
        raise _lib.HipKernelError(f"composite: edited {tuple(edited.shape)} / original {tuple(original.shape)} must be [N,3,H,W] and mask "
                                  f"{tuple(mask.shape)} [N,H,W]")
    if out is None:
        out = torch.empty_like(edited)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == edited.shape):
        raise _lib.HipKernelError("composite: out must be a contiguous CUDA float32 tensor shaped like edited")
    N, _, H, W = edited.shape
    check(lib.insv2v_composite(edited.data_ptr(), original.data_ptr(), mask.data_ptr(), out.data_ptr(), N, H, W, _stream()), "insv2v_composite")
    return out


def mask_track_step(f_prev, v_prev, b, c, m, *, alpha=0.01, beta=0.5, fill=0.0, out=None):
    """One step of the key-frame mask chain (insv2v_mask_track_step; DESIGN.md section 19, tests/masktrack_ref.py is the definition):
    fp32 ``f_prev`` [N,2,H,W] / ``v_prev`` [N,H,W] of the chain's previous frame, ``b`` [N,2,H,W] the flow on this frame into the previous
    one, ``c`` the opposite flow or None (no consistency check), ``m`` [N,H,W] the key mask -> (F [N,2,H,W], V [N,H,W], mask [N,H,W]).
    ``out``: that triple, preallocated; the entry refuses outputs that overlap an input or one another."""
    lib = _lib.load()
    N, _, H, W = b.shape if torch.is_tensor(b) and b.dim() == 4 else (0, 0, 0, 0)
    for name, t, shape in (("f_prev", f_prev, (N, 2, H, W)), ("v_prev", v_prev, (N, H, W)), ("b", b, (N, 2, H, W)), ("c", c, (N, 2, H, W)),
                           ("m", m, (N, H, W))):
        if t is None and name == "c":
            continue
        _req(t, torch.float32, "mask_track_step." + name)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.HipKernelError(f"mask_track_step: {name} {tuple(t.shape)} must be a contiguous {shape}")
    if out is None:
        out = (torch.empty_like(b), torch.empty_like(v_prev), torch.empty_like(v_prev))
    for name, t, shape in zip(("F", "V", "mask"), out, ((N, 2, H, W), (N, H, W), (N, H, W))):
        _req(t, torch.float32, "mask_track_step.out." + name)
        if tuple(t.shape) != shape or not t.is_contiguous():
            raise _lib.HipKernelError(f"mask_track_step: out {name} {tuple(t.shape)} must be a contiguous {shape}")
    d = MaskTrackDesc()
    d.f_prev, d.v_prev, d.b, d.c, d.m = f_prev.data_ptr(), v_prev.data_ptr(), b.data_ptr(), _ptr(c), m.data_ptr()
    d.f_out, d.v_out, d.mask_out = (t.data_ptr() for t in out)
    d.N, d.H, d.W, d.alpha, d.beta, d.fill = N, H, W, alpha, beta, fill
    check(lib.insv2v_mask_track_step(_byref(d), _stream()), "insv2v_mask_track_step")
    return tuple(out)


def add_noise(z, noise, ka, kb):
    """ka * z + kb * noise (fp32, any shape): the source latent re-noised to the level (ka, kb) = (sqrt(a), sqrt(1 - a))."""
    lib = _lib.load()
    _req(z, torch.float32, "add_noise.z"), _req(noise, torch.float32, "add_noise.noise")
    if z.shape != noise.shape:
        raise _lib.HipKernelError(f"add_noise: z {tuple(z.shape)} and noise {tuple(noise.shape)} differ")
    z, noise = z.contiguous(), noise.contiguous()
    out = torch.empty_like(z)
    check(lib.insv2v_add_noise(z.data_ptr(), noise.data_ptr(), out.data_ptr(), z.numel(), ka, kb, _stream()), "insv2v_add_noise")
    return out


def build_unet_input_noised(latent, img_cond, out, t_out, timestep, ka, kb, *, noise=None, seed=None, stream=0, branch_rows=0, t_stride=0):
    """``build_unet_input`` for the three CFG branches whose latent is ``ka * latent + kb * noise`` (insv2v_build_unet_input_noised):
    ``noise`` fp32 [F,4,h,w], or - ``seed`` / ``stream`` - generated inside the kernel from the seeded stream (element = flat index of
    [F,4,h,w]); passing both, or neither, is refused.  Bit-identical to ``add_noise`` (+ ``randn``) followed by ``build_unet_input``."""
    lib = _lib.load()
    _req(latent, torch.float32, "build_unet_input_noised.latent"), _req(img_cond, torch.float32, "build_unet_input_noised.img_cond")
    if (noise is None) == (seed is None):
        raise _lib.HipKernelError("build_unet_input_noised: pass noise or seed, exactly one of them")
    shape = tuple(latent.shape[-4:])
    for name, t in (("latent", latent), ("img_cond", img_cond), ("noise", noise)):
        if t is not None and (tuple(t.shape[-4:]) != shape or t.numel() != math.prod(shape) or not t.is_contiguous()):
            raise _lib.HipKernelError(f"build_unet_input_noised: {name} {tuple(t.shape)} must be contiguous and shaped {shape}")
    if noise is not None:
        _req(noise, torch.float32, "build_unet_input_noised.noise")
    F, _, h, w = shape
    rows = F * h * w
    _req(out, torch.float16, "build_unet_input_noised.out")
    if out.dim() != 2 or not out.is_contiguous() or out.shape[0] < 2 * (branch_rows or rows) + rows:   # the three branches must lie inside out
        raise _lib.HipKernelError(f"build_unet_input_noised: out {tuple(out.shape)} does not hold 3 branches of {rows} rows at stride {branch_rows or rows}")
    if t_out is not None and (_req(t_out, torch.float32, "build_unet_input_noised.t_out").numel() < 2 * (t_stride or 1) + 1 or not t_out.is_contiguous()):
        raise _lib.HipKernelError(f"build_unet_input_noised: t_out {tuple(t_out.shape)} does not hold 3 entries at stride {t_stride or 1}")
    check(lib.insv2v_build_unet_input_noised(latent.data_ptr(), img_cond.data_ptr(), _ptr(noise), out.data_ptr(), _ptr(t_out), float(timestep),
                                             ka, kb, as_int64(seed) if seed is not None else 0, as_int64(stream, "stream"),
                                             int(seed is not None), F, h, w, out.shape[-1], branch_rows, t_stride, _stream()),
          "insv2v_build_unet_input_noised")
    return out


def eps_absdiff_accum(eps, acc, scale, *, accumulate, branch_stride=0):
    """acc [F,h,w] (``accumulate``: +=, else =) ``scale`` * sum_c |eps3 - eps2| from the UNet's channels-last fp32 output ``eps`` (a view
    that starts at the clip's first branch; ``branch_stride`` fp32 elements between the branches as for ``cfg_step``, 0 = back to back).
    Branch 0 is not read."""
    lib = _lib.load()
    _req(eps, torch.float32, "eps_absdiff_accum.eps"), _req(acc, torch.float32, "eps_absdiff_accum.acc")
    if acc.dim() < 3 or not acc.is_contiguous() or acc.numel() != math.prod(acc.shape[-3:]):
        raise _lib.HipKernelError(f"eps_absdiff_accum: acc {tuple(acc.shape)} must be a contiguous [F,h,w]")
    F, h, w = acc.shape[-3:]
    bs = branch_stride if branch_stride > 0 else 4 * F * h * w
    if not eps.is_contiguous() or eps.numel() < 2 * bs + 4 * F * h * w:
        raise _lib.HipKernelError(f"eps_absdiff_accum: eps ({eps.numel()} elements) does not hold branches 1 and 2 of [{F},{h},{w},4] at stride {bs}")
    check(lib.insv2v_eps_absdiff_accum(eps.data_ptr(), acc.data_ptr(), F, h, w, branch_stride, scale, int(bool(accumulate)), _stream()),
          "insv2v_eps_absdiff_accum")
    return acc


def automask_finish(raw, *, clamp_ratio=3.0, threshold=0.5, smooth=True, dilate=1):
    """raw fp32 [T,h,w] -> (soft [T,h,w], mask_latent [T,h,w] of 0 / 1, mask [T,8h,8w]): insv2v_automask_finish - the video's mean (a
    fixed-order reduction), ``min(raw, r mean) / (r mean)``, the optional temporal + spatial binomial smoothing, ``> threshold``, the
    spatial dilation and the 8 x 8 replication (tests/automask_ref.py is the definition)."""
    lib = _lib.load()
    _req(raw, torch.float32, "automask_finish.raw")
    if raw.dim() != 3 or not raw.is_contiguous():
        raise _lib.HipKernelError(f"automask_finish: raw {tuple(raw.shape)} must be a contiguous [T,h,w]")
    T, h, w = raw.shape
    soft, mask_latent = torch.empty_like(raw), torch.empty_like(raw)
    mask = torch.empty((T, 8 * h, 8 * w), device=raw.device, dtype=torch.float32)
    nbytes = lib.insv2v_automask_workspace_bytes(T, h, w)
    if nbytes <= 0:
        raise _lib.HipKernelError(f"automask_finish: no workspace size for raw {tuple(raw.shape)}")
    ws = torch.empty((nbytes + 3) // 4, device=raw.device, dtype=torch.float32)
    check(lib.insv2v_automask_finish(raw.data_ptr(), soft.data_ptr(), mask_latent.data_ptr(), mask.data_ptr(), ws.data_ptr(), ws.numel() * 4,
                                     T, h, w, clamp_ratio, threshold, int(bool(smooth)), int(dilate), _stream()), "insv2v_automask_finish")
    return soft, mask_latent, mask


def _fill_step_desc(d, eps_in, latent, *, nbranch, text_cfg=1.0, img_cfg=1.0, sqrt_a=1.0, sqrt_1ma=0.0, coef=(0, 0, 0, 0),
                    latent_out=None, pred_x0=None, eps_out=None, latent_ref=None, correct=0, delta_q=None, noise=None,
                    rescale_stats=None, guidance_rescale=0.0, branch_stride=0, noise_seed=None, noise_stream=0):
    """The fields StepDesc and MStepDesc share."""
    F, _, h, w = latent.shape[-4:]
    d.eps_in, d.latent = _req(eps_in, torch.float32, "eps_in").data_ptr(), _req(latent, torch.float32, "latent").data_ptr()
    d.latent_ref, d.delta_q, d.noise, d.rescale_stats = _ptr(latent_ref), _ptr(delta_q), _ptr(noise), _ptr(rescale_stats)
    d.latent_out, d.pred_x0, d.eps_out = _ptr(latent_out), _ptr(pred_x0), _ptr(eps_out)
    d.nbranch, d.F, d.h, d.w, d.correct = nbranch, F, h, w, correct
    d.R = latent_ref.shape[-4] if latent_ref is not None else 0
    d.text_cfg, d.img_cfg, d.sqrt_a, d.sqrt_1ma = text_cfg, img_cfg, sqrt_a, sqrt_1ma
    d.c_x0, d.c_eps, d.c_xt, d.c_noise = coef
    d.guidance_rescale, d.branch_stride = guidance_rescale, branch_stride
    if noise_seed is not None:
        d.noise_seed, d.noise_stream, d.noise_on = as_int64(noise_seed), as_int64(noise_stream, "stream"), 1
    return d


def cfg_stats(eps_in, stats, F, h, w, text_cfg, img_cfg, branch_stride=0):
    lib = _lib.load()
    check(lib.insv2v_cfg_stats(eps_in.data_ptr(), stats.data_ptr(), F, h, w, text_cfg, img_cfg, branch_stride, _stream()), "insv2v_cfg_stats")


def warp_image(image, flow):
    lib = _lib.load()
    _req(image, torch.float32, "warp.image"), _req(flow, torch.float32, "warp.flow")
    image, flow = image.contiguous(), flow.contiguous()
    N, Cc, H, W = image.shape
    out = torch.empty_like(image)
    check(lib.insv2v_warp_image(image.data_ptr(), flow.data_ptr(), out.data_ptr(), N, Cc, H, W, _stream()), "insv2v_warp_image")
    return out


def resize_flow(flow, size):
    lib = _lib.load()
    _req(flow, torch.float32, "resize_flow.flow")
    flow = flow.contiguous()
    N, _, h, w = flow.shape
    H, W = size
    out = torch.empty((N, 2, H, W), device=flow.device, dtype=torch.float32)
    check(lib.insv2v_resize_flow(flow.data_ptr(), out.data_ptr(), N, h, w, H, W, _stream()), "insv2v_resize_flow")
    return out


def flow_correction(eps_cfg, latent, latent_ref, flows, sqrt_a, sqrt_1ma):
    lib = _lib.load()
    F, _, h, w = latent.shape[-4:]
    R = latent_ref.shape[-4]
    out = torch.empty((F - R, 4, h, w), device=latent.device, dtype=torch.float32)
    check(lib.insv2v_flow_correction(eps_cfg.data_ptr(), latent.data_ptr(), latent_ref.data_ptr(), flows.data_ptr(),
                                     out.data_ptr(), F, R, h, w, sqrt_a, sqrt_1ma, _stream()), "insv2v_flow_correction")
    return out


def nchw_to_nhwc_f16(x, ldo, scale=1.0):
    lib = _lib.load()
    _req(x, torch.float32, "nchw_to_nhwc.x")
    x = x.contiguous()
    N, Cc, H, W = x.shape
    out = torch.empty((N * H * W, ldo), device=x.device, dtype=torch.float16)
    check(lib.insv2v_nchw_to_nhwc_f16(x.data_ptr(), out.data_ptr(), N, Cc, H, W, ldo, scale, _stream()), "insv2v_nchw_to_nhwc_f16")
    return out


def nhwc_to_nchw_f32(x, N, Cc, H, W, scale=1.0):
    lib = _lib.load()
    out = torch.empty((N, Cc, H, W), device=x.device, dtype=torch.float32)
    check(lib.insv2v_nhwc_to_nchw_f32(x.data_ptr(), int(x.dtype == torch.float32), out.data_ptr(), N, Cc, H, W,
                                      x.stride(0), scale, _stream()), "insv2v_nhwc_to_nchw_f32")
    return out


def posterior_sample(moments, noise, N, H, W, scale, seed=None, stream=0, offset=0):
    """``seed`` (with ``noise=None``): the noise is generated inside the kernel, element i of the sample from element ``offset`` + i of the
    normal stream (seed, stream)."""
    lib = _lib.load()
    _req(moments, torch.float32, "posterior.moments")
    z = torch.empty((N, 4, H, W), device=moments.device, dtype=torch.float32)
    if seed is not None:
        if noise is not None:
            raise _lib.HipKernelError("posterior_sample: pass noise or seed, not both")
        check(lib.insv2v_posterior_sample_seeded(moments.data_ptr(), z.data_ptr(), N, H, W, moments.stride(0), scale,
                                                 as_int64(seed), as_int64(stream, "stream"), int(offset), _stream()), "insv2v_posterior_sample_seeded")
        return z
    _req(noise, torch.float32, "posterior.noise")
    check(lib.insv2v_posterior_sample(moments.data_ptr(), noise.contiguous().data_ptr(), z.data_ptr(), N, H, W,
                                      moments.stride(0), scale, _stream()), "insv2v_posterior_sample")
    return z


def randn(shape_or_out, seed, stream, offset=0, raw=False, device=None):
    """Elements [offset, offset + n) of the seeded stream (seed, stream) (include/insv2v_hip.h, "seeded noise"): fp32 normals, or with
    ``raw`` the 32-bit words' bit patterns as int32.  ``shape_or_out``: a shape (a new tensor on ``device`` / the current GPU is
    returned) or a contiguous CUDA tensor to fill (float32; int32 also with ``raw``)."""
    lib = _lib.load()
    if torch.is_tensor(shape_or_out):
        out = shape_or_out
        if not (out.is_cuda and out.is_contiguous() and (out.dtype == torch.float32 or (raw and out.dtype == torch.int32))):
            raise _lib.HipKernelError(f"randn: expected a contiguous CUDA float32 tensor, got {out.device} {out.dtype}")
    else:
        shape = (shape_or_out,) if isinstance(shape_or_out, int) else tuple(shape_or_out)
        out = torch.empty(shape, device=device if device is not None else torch.device("cuda", torch.cuda.current_device()),
                          dtype=torch.int32 if raw else torch.float32)
    check(lib.insv2v_randn(out.data_ptr(), out.numel(), as_int64(seed), as_int64(stream, "stream"), int(offset), int(bool(raw)), _stream()),
          "insv2v_randn")
    return out


# ----------------------------------------------------------------------------- optical-flow estimator (insv2v/raft.py)
def im2col(x, geom, C, kh, kw, stride=1, pad=(0, 0), x2=None):
    """x fp16 [N*IH*IW, C1] (+ x2 [.., C - C1]) -> fp16 [N*OH*OW, kh*kw*C] and the output geometry (N, OH, OW)."""
    lib = _lib.load()
    _req(x, torch.float16, "im2col.x")
    N, IH, IW = geom
    OH, OW = (IH + 2 * pad[0] - kh) // stride + 1, (IW + 2 * pad[1] - kw) // stride + 1
    out = torch.empty((N * OH * OW, kh * kw * C), device=x.device, dtype=torch.float16)
    d = _lib.Im2colDesc()
    d.x, d.out, d.ldx, d.ldo = x.data_ptr(), out.data_ptr(), x.stride(0), out.stride(0)
    if x2 is not None:
        _req(x2, torch.float16, "im2col.x2")
        d.x2, d.ldx2, d.C1 = x2.data_ptr(), x2.stride(0), C - x2.shape[1]
    else:
        d.C1 = C
    d.N, d.IH, d.IW, d.C, d.KH, d.KW = N, IH, IW, C, kh, kw
    d.stride_h = d.stride_w = stride
    d.pad_h, d.pad_w, d.OH, d.OW = pad[0], pad[1], OH, OW
    with _timed("im2col", 0.0, ("im2col", N * OH * OW, kh * kw * C)):
        check(lib.insv2v_im2col(_byref(d), _stream()), "insv2v_im2col")
    return out, (N, OH, OW)


def instance_norm(x, N, HW, relu=False, eps=1e-5):
    """nn.InstanceNorm2d (no affine) (+ ReLU) over channels-last fp16 [N*HW, C]; returns a new tensor."""
    lib = _lib.load()
    _req(x, torch.float16, "instance_norm.x")
    Cc = x.shape[1]
    nchunks = max(1, min(64, HW // 64))
    part = torch.empty((N * nchunks * Cc * 2,), device=x.device, dtype=torch.float32)
    y = torch.empty((x.shape[0], Cc), device=x.device, dtype=torch.float16)
    with _timed("instnorm", 0.0, ("instnorm", N, HW, Cc)):
        check(lib.insv2v_instance_norm(x.data_ptr(), y.data_ptr(), part.data_ptr(), N, HW, Cc, x.stride(0), y.stride(0), nchunks, eps,
                                       int(relu), _stream()), "insv2v_instance_norm")
    return y


def ew(op, a, b=None, c=None, out=None):
    """Element-wise op on fp16 [rows, C] views (column slices of wider buffers are fine): see INSV2V_EW_* in the header."""
    lib = _lib.load()
    _req(a, torch.float16, "ew.a")
    rows, Cc = a.shape
    if out is None:
        out = torch.empty((rows, Cc), device=a.device, dtype=torch.float16)
    check(lib.insv2v_ew(op, a.data_ptr(), _ptr(b), _ptr(c), out.data_ptr(), rows, Cc, a.stride(0), b.stride(0) if b is not None else 0,
                        c.stride(0) if c is not None else 0, out.stride(0), _stream()), "insv2v_ew")
    return out


def avgpool2x2(x, n, h, w):
    lib = _lib.load()
    _req(x, torch.float32, "avgpool.x")
    y = torch.empty((n, h // 2, w // 2), device=x.device, dtype=torch.float32)
    check(lib.insv2v_avgpool2x2(x.data_ptr(), y.data_ptr(), n, h, w, _stream()), "insv2v_avgpool2x2")
    return y


def corr_lookup(pyramid, coords, B, h, w, radius, ldo):
    lib = _lib.load()
    out = torch.empty((B * h * w, ldo), device=coords.device, dtype=torch.float16)
    d = _lib.CorrLookupDesc()
    ptrs = [t.data_ptr() for t in pyramid] + [None] * (4 - len(pyramid))
    d.pyr0, d.pyr1, d.pyr2, d.pyr3 = ptrs
    d.coords, d.out, d.ldo = _req(coords, torch.float32, "corr_lookup.coords").data_ptr(), out.data_ptr(), ldo
    d.B, d.h, d.w, d.levels, d.radius = B, h, w, len(pyramid), radius
    with _timed("corr_lookup", 0.0, ("corr_lookup", B * h * w, ldo)):
        check(lib.insv2v_corr_lookup(_byref(d), _stream()), "insv2v_corr_lookup")
    return out


def raft_flow_rows(coords1, delta, rows, B, h, w):
    """coords1 [B,2,h,w] fp32 += delta rows (fp32 [B*h*w, ld], or None); rows (fp16 [B*h*w, n] view or None) <- coords1 - pixel grid."""
    lib = _lib.load()
    check(lib.insv2v_raft_flow_rows(coords1.data_ptr(), _ptr(delta), delta.stride(0) if delta is not None else 0, _ptr(rows),
                                    rows.stride(0) if rows is not None else 0, rows.shape[1] if rows is not None else 0, B, h, w, _stream()),
          "insv2v_raft_flow_rows")


def convex_upsample(coords1, mask, B, h, w):
    lib = _lib.load()
    _req(mask, torch.float16, "convex_upsample.mask")
    out = torch.empty((B, 2, 8 * h, 8 * w), device=coords1.device, dtype=torch.float32)
    check(lib.insv2v_convex_upsample(coords1.data_ptr(), mask.data_ptr(), mask.stride(0), out.data_ptr(), B, h, w, _stream()),
          "insv2v_convex_upsample")
    return out


# ----------------------------------------------------------------------------- scoring an edit with CLIP (insv2v/clip_score.py)
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)   # clip_similarity.py:19-20
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def clip_preprocess(frames, size, patch, ld=None, in_scale=1.0, in_shift=0.0, mean=CLIP_MEAN, std=CLIP_STD, out=None):
    """frames [n,3,H,W] fp16 / fp32 (any strided view) -> fp16 patch rows [n * (size/patch)^2, ld] of the bicubic-resized, mean / std
    normalised size x size image (insv2v_clip_preprocess); ld defaults to 3 * patch^2 rounded up to 64, pad columns are zeros."""
    lib = _lib.load()
    if not torch.is_tensor(frames) or not frames.is_cuda or frames.dtype not in (torch.float16, torch.float32):
        raise _lib.HipKernelError("clip_preprocess.frames: expected a CUDA float16 / float32 tensor")
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise _lib.HipKernelError(f"clip_preprocess: frames {tuple(frames.shape)} must be [n,3,H,W]")
    n, _, H, W = frames.shape
    if ld is None:
        ld = -(-3 * patch * patch // 64) * 64
    g = size // patch if patch > 0 else 0
    if out is None:
        out = torch.empty((max(n * g * g, 0), max(ld, 0)), device=frames.device, dtype=torch.float16)
    else:
        _req(out, torch.float16, "clip_preprocess.out")
        if out.dim() != 2 or out.stride(1) != 1 or out.stride(0) != ld or out.shape[0] < n * g * g or out.shape[1] < min(ld, 3 * patch * patch):
            raise _lib.HipKernelError(f"clip_preprocess: out {tuple(out.shape)} (row stride {out.stride(0)}) does not hold {n * g * g} rows of ld {ld}")
    d = _lib.ClipPreprocessDesc()
    d.x, d.out, d.ld = frames.data_ptr() or None, out.data_ptr() or None, ld
    d.stride_n, d.stride_c, d.stride_h, d.stride_w = frames.stride()
    d.n, d.H, d.W, d.S, d.P, d.x_fp32 = n, H, W, size, patch, int(frames.dtype == torch.float32)
    d.in_scale, d.in_shift = in_scale, in_shift
    d.mean[:], d.std[:] = [float(v) for v in mean], [float(v) for v in std]
    with _timed("elementwise", 0.0, ("clip_pre", n, H, W, size)):
        check(lib.insv2v_clip_preprocess(_byref(d), _stream()), "insv2v_clip_preprocess")
    return out


def clip_scores(img0, img1, txt0, txt1, eps=1e-8):
    """Features img0 / img1 [n, D] and txt0 / txt1 [D] (one prompt for every frame) or [n, D], all float16 or all float32 ->
    fp32 [n, 5] = (sim_0, sim_1, sim_direction, sim_image, consistency) per frame (insv2v_clip_scores)."""
    lib = _lib.load()
    dt = img0.dtype if torch.is_tensor(img0) else None
    if dt not in (torch.float16, torch.float32):
        raise _lib.HipKernelError("clip_scores: features must be CUDA float16 or float32 tensors")
    for name, t in (("img0", img0), ("img1", img1), ("txt0", txt0), ("txt1", txt1)):
        _req(t, dt, "clip_scores." + name)
        if t.stride(-1) != 1:
            raise _lib.HipKernelError(f"clip_scores: {name} rows must be contiguous")
    if img0.dim() != 2 or img1.shape != img0.shape:
        raise _lib.HipKernelError(f"clip_scores: img0 {tuple(img0.shape)} and img1 {tuple(img1.shape)} must both be [n, D]")
    n, D = img0.shape
    if txt0.shape != txt1.shape or tuple(txt0.shape) not in ((D,), (1, D), (n, D)):
        raise _lib.HipKernelError(f"clip_scores: txt0 {tuple(txt0.shape)} / txt1 {tuple(txt1.shape)} must be [{D}] or [{n}, {D}]")
    ldt = 0
    if txt0.dim() == 2 and txt0.shape[0] == n and n > 1:
        if txt0.stride(0) != txt1.stride(0):
            txt1 = txt1.contiguous()
            txt0 = txt0.contiguous()
        ldt = txt0.stride(0)
    out = torch.empty((n, 5), device=img0.device, dtype=torch.float32)
    with _timed("elementwise", 0.0, ("clip_scores", n, D)):
        check(lib.insv2v_clip_scores(img0.data_ptr(), img1.data_ptr(), txt0.data_ptr(), txt1.data_ptr(), int(dt == torch.float32),
                                     img0.stride(0), img1.stride(0), ldt, n, D, eps, out.data_ptr(), _stream()), "insv2v_clip_scores")
    return out


def l2_normalize(x):
    """x [n, D] float16 / float32 -> fp32 [n, D] = x / |x| per row (insv2v_l2_normalize)."""
    lib = _lib.load()
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype not in (torch.float16, torch.float32) or x.dim() != 2 or x.stride(1) != 1:
        raise _lib.HipKernelError("l2_normalize: expected a CUDA float16 / float32 [n, D] tensor with contiguous rows")
    out = torch.empty(tuple(x.shape), device=x.device, dtype=torch.float32)
    check(lib.insv2v_l2_normalize(x.data_ptr(), int(x.dtype == torch.float32), x.stride(0), out.data_ptr(), out.stride(0), x.shape[0],
                                  x.shape[1], _stream()), "insv2v_l2_normalize")
    return out


# ----------------------------------------------------------------------------- scoring an edit in pixel space (insv2v/pixel_score.py)
FIDELITY_KEYS = ("se", "se_in", "se_out", "w_in", "w_out", "ssim", "ssim_in", "ssim_out", "wc_in", "wc_out")   # insv2v_frame_fidelity's sums


def _frames_view(v, t, name, scale, shift):
    """Fill an insv2v_frames_view from a [T,3,H,W] fp16 / fp32 CUDA tensor (any view whose rows are contiguous)."""
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype not in (torch.float16, torch.float32):
        raise _lib.HipKernelError(f"{name}: expected a CUDA float16 / float32 tensor")
    if t.dim() != 4 or t.shape[1] != 3 or (t.shape[3] > 1 and t.stride(3) != 1):
        raise _lib.HipKernelError(f"{name}: {tuple(t.shape)} (strides {t.stride()}) must be [T,3,H,W] with contiguous rows")
    v.p, v.fp32, v.scale, v.shift = t.data_ptr() or None, int(t.dtype == torch.float32), scale, shift
    v.stride_t, v.stride_c, v.stride_h = t.stride(0), t.stride(1), t.stride(2)
    return tuple(t.shape)


def _plain(t, shape, name, dtype=torch.float32):
    _req(t, dtype, name)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise _lib.HipKernelError(f"{name}: {tuple(t.shape)} must be a contiguous {tuple(shape)}")
    return t


def _score_workspace(nbytes, device, workspace, name):
    if nbytes <= 0:
        raise _lib.HipKernelError(f"{name}: no workspace size for these frames")
    if workspace is None:
        workspace = torch.empty(nbytes // 8, device=device, dtype=torch.float64)
    else:
        _req(workspace, torch.float64, name + ".workspace")
        if not workspace.is_contiguous():
            raise _lib.HipKernelError(f"{name}: the workspace must be contiguous")
    return workspace


def warp_error_workspace_elems(T, H, W):
    """fp64 elements of workspace ``warp_error`` needs (insv2v_warp_error_workspace_bytes / 8); <= 0: the entry refuses the size."""
    n = _lib.load().insv2v_warp_error_workspace_bytes(T, H, W)
    return n // 8 if n > 0 else n


def frame_fidelity_workspace_elems(T, H, W):
    n = _lib.load().insv2v_frame_fidelity_workspace_bytes(T, H, W)
    return n // 8 if n > 0 else n


def frame_fidelity_tile():
    """(rows, columns) of SSIM centres one workgroup of insv2v_frame_fidelity owns."""
    r, c = C.c_int32(), C.c_int32()
    _lib.load().insv2v_frame_fidelity_tile(_byref(r), _byref(c))
    return r.value, c.value


def warp_error(frames, fwd, bwd=None, region=None, *, scale=1.0, shift=0.0, alpha=0.01, beta=0.5, return_maps=False, out=None, workspace=None):
    """insv2v_warp_error: ``frames`` [T,3,H,W] fp16 / fp32 (any view with contiguous rows; ``clamp(x * scale + shift, 0, 1)`` as it is
    read), ``fwd`` / ``bwd`` [T-1,2,H,W] fp32 (``bwd`` None: no consistency check), ``region`` [T,H,W] fp32 or None -> fp64 sums
    [T-1,3] = (sum valid w err, sum valid w, valid count), and with ``return_maps`` also (err_map, valid_map) [T-1,H,W] fp32.
    ``out``: the preallocated (sums, err_map or None, valid_map or None)."""
    lib = _lib.load()
    d = _lib.WarpErrorDesc()
    T, _, H, W = _frames_view(d.a, frames, "warp_error.frames", scale, shift)
    P = max(T - 1, 0)
    _plain(fwd, (P, 2, H, W), "warp_error.fwd")
    if bwd is not None:
        _plain(bwd, (P, 2, H, W), "warp_error.bwd")
    if region is not None:
        _plain(region, (T, H, W), "warp_error.region")
    if out is None:
        maps = [torch.empty((P, H, W), device=frames.device, dtype=torch.float32) for _ in range(2)] if return_maps else [None, None]
        out = (torch.empty((P, 3), device=frames.device, dtype=torch.float64), *maps)
    sums, err_map, valid_map = out
    _plain(sums, (P, 3), "warp_error.out.sums", torch.float64)
    for name, t in (("err_map", err_map), ("valid_map", valid_map)):
        if t is not None:
            _plain(t, (P, H, W), "warp_error.out." + name)
    ws = _score_workspace(lib.insv2v_warp_error_workspace_bytes(T, H, W), frames.device, workspace, "warp_error")
    d.fwd, d.bwd, d.w, d.sums, d.err_map, d.valid_map = fwd.data_ptr() or None, _ptr(bwd), _ptr(region), sums.data_ptr() or None, _ptr(err_map), _ptr(valid_map)
    d.workspace, d.workspace_bytes = ws.data_ptr() or None, ws.numel() * 8
    d.T, d.H, d.W, d.alpha, d.beta = T, H, W, alpha, beta
    check(lib.insv2v_warp_error(_byref(d), _stream()), "insv2v_warp_error")
    return (sums, err_map, valid_map) if return_maps else sums


def frame_fidelity(x, y, region=None, *, x_affine=(1.0, 0.0), y_affine=(1.0, 0.0), out=None, workspace=None):
    """insv2v_frame_fidelity: source ``x`` and edit ``y`` [T,3,H,W] (each fp16 or fp32, with its own strides and (scale, shift)),
    ``region`` [T,H,W] fp32 or None -> fp64 sums [T, 10] in the order of ``FIDELITY_KEYS``."""
    lib = _lib.load()
    d = _lib.FidelityDesc()
    shape = _frames_view(d.x, x, "frame_fidelity.x", *x_affine)
    if _frames_view(d.y, y, "frame_fidelity.y", *y_affine) != shape:
        raise _lib.HipKernelError(f"frame_fidelity: x {shape} and y {tuple(y.shape)} differ")
    T, _, H, W = shape
    if region is not None:
        _plain(region, (T, H, W), "frame_fidelity.region")
    if out is None:
        out = torch.empty((T, _lib.FIDELITY_K), device=x.device, dtype=torch.float64)
    _plain(out, (T, _lib.FIDELITY_K), "frame_fidelity.out", torch.float64)
    ws = _score_workspace(lib.insv2v_frame_fidelity_workspace_bytes(T, H, W), x.device, workspace, "frame_fidelity")
    d.w, d.sums, d.workspace, d.workspace_bytes = _ptr(region), out.data_ptr() or None, ws.data_ptr() or None, ws.numel() * 8
    d.T, d.H, d.W = T, H, W
    check(lib.insv2v_frame_fidelity(_byref(d), _stream()), "insv2v_frame_fidelity")
    return out


# ----------------------------------------------------------------------------- stabilizing an edit (insv2v/temporal_filter.py)
def temporal_filter(edited, guide, flow, valid, offsets, *, sigma=0.1, strength=1.0, guide_affine=(1.0, 0.0), out=None):
    """insv2v_temporal_filter (tests/temporal_filter_ref.py is the definition): ``edited`` and ``guide`` [T,3,H,W],
    each fp16 or fp32 and any view with contiguous rows (the guide is read as ``clamp(x * scale + shift, 0, 1)``), ``flow`` [K,T,2,H,W] and
    ``valid`` [K,T,H,W] fp32 contiguous, ``offsets`` the K neighbour offsets -> the filtered frames [T,3,H,W] in ``edited``'s dtype.
    ``out``: preallocated, any view with contiguous rows; the entry refuses one that overlaps an input."""
    lib = _lib.load()
    d = _lib.TemporalFilterDesc()
    shape = _frames_view(d.e, edited, "temporal_filter.edited", 1.0, 0.0)
    if _frames_view(d.a, guide, "temporal_filter.guide", *guide_affine) != shape:
        raise _lib.HipKernelError(f"temporal_filter: edited {shape} and guide {tuple(guide.shape)} differ")
    T, _, H, W = shape
    offsets = [int(k) for k in offsets]
    K = len(offsets)
    if K > _lib.TFILTER_MAX_K:
        raise _lib.HipKernelError(f"temporal_filter: {K} neighbours, at most {_lib.TFILTER_MAX_K}")
    _plain(flow, (K, T, 2, H, W), "temporal_filter.flow")
    _plain(valid, (K, T, H, W), "temporal_filter.valid")
    if out is None:
        out = torch.empty(shape, device=edited.device, dtype=edited.dtype)
    ov = _lib.FramesView()
    if _frames_view(ov, out, "temporal_filter.out", 1.0, 0.0) != shape or out.dtype != edited.dtype:
        raise _lib.HipKernelError(f"temporal_filter: out {tuple(out.shape)} {out.dtype} must be {shape} {edited.dtype}")
    d.flow, d.valid, d.out = flow.data_ptr() or None, valid.data_ptr() or None, ov.p
    d.out_stride_t, d.out_stride_c, d.out_stride_h = ov.stride_t, ov.stride_c, ov.stride_h
    for i, k in enumerate(offsets):
        d.offsets[i] = k
    d.K, d.T, d.H, d.W, d.sigma, d.strength = K, T, H, W, sigma, strength
    check(lib.insv2v_temporal_filter(_byref(d), _stream()), "insv2v_temporal_filter")
    return out


# ----------------------------------------------------------------------------- filling between key frames (insv2v/keyfill.py)
def keyframe_fill(source, edited_keys, flow, valid, key_frame, frames, slots, weights, *, sigma=0.1, mode="residual", guide_affine=(1.0, 0.0),
                  out=None, conf=None):
    """insv2v_keyframe_fill (tests/keyfill_ref.py is the definition): ``source`` [T,3,H,W] and ``edited_keys``
    [Tk,3,H,W], each fp16 or fp32 and any view with contiguous rows (the source is read raw for the residual and as ``clamp(x * scale +
    shift, 0, 1)`` for the photometric weight), ``flow`` [n,2,2,H,W] and ``valid`` [n,2,H,W] fp32 contiguous; the host tables
    ``key_frame`` (Tk frame indices), ``frames`` (n in-between frames), ``slots`` (n pairs of key slots, -1 = no such side) and
    ``weights`` (n pairs of temporal weights) -> (out, conf): ``out`` the FULL-RATE [T,3,H,W] in ``edited_keys``' dtype, of which only
    the rows of ``frames`` are written (preallocated: any view with contiguous rows, its other rows are not touched; default: a new
    tensor whose other rows are uninitialised), ``conf`` [n,H,W] fp32 (preallocated, or ``False``: not computed)."""
    lib = _lib.load()
    d = _lib.KeyfillDesc()
    T, _, H, W = _frames_view(d.a, source, "keyframe_fill.source", *guide_affine)
    Tk = _frames_view(d.e, edited_keys, "keyframe_fill.edited_keys", 1.0, 0.0)[0]
    if tuple(edited_keys.shape[1:]) != (3, H, W):
        raise _lib.HipKernelError(f"keyframe_fill: source {tuple(source.shape)} and edited_keys {tuple(edited_keys.shape)} differ in frame size")
    if mode not in _lib.KEYFILL_MODES:
        raise ValueError(f"keyframe_fill: mode {mode!r} is neither 'residual' nor 'warp'")
    key_frame, frames = [int(k) for k in key_frame], [int(t) for t in frames]
    slots, weights = [[int(v) for v in s] for s in slots], [[float(v) for v in w] for w in weights]
    n = len(frames)
    if len(key_frame) != Tk or len(slots) != n or len(weights) != n or any(len(s) != 2 for s in slots) or any(len(w) != 2 for w in weights):
        raise _lib.HipKernelError(f"keyframe_fill: {len(key_frame)} key frames for {Tk} slots, {len(slots)} slot pairs and {len(weights)} weight pairs for {n} frames")
    _plain(flow, (n, 2, 2, H, W), "keyframe_fill.flow")
    _plain(valid, (n, 2, H, W), "keyframe_fill.valid")
    if out is None:
        out = torch.empty((T, 3, H, W), device=edited_keys.device, dtype=edited_keys.dtype)
    ov = _lib.FramesView()
    if _frames_view(ov, out, "keyframe_fill.out", 1.0, 0.0) != (T, 3, H, W) or out.dtype != edited_keys.dtype:
        raise _lib.HipKernelError(f"keyframe_fill: out {tuple(out.shape)} {out.dtype} must be {(T, 3, H, W)} {edited_keys.dtype}")
    if conf is None:
        conf = torch.empty((n, H, W), device=edited_keys.device, dtype=torch.float32)
    if conf is not False:
        _plain(conf, (n, H, W), "keyframe_fill.conf")
    d.flow, d.valid, d.out, d.conf = flow.data_ptr() or None, valid.data_ptr() or None, ov.p, None if conf is False else (conf.data_ptr() or None)
    d.out_stride_t, d.out_stride_c, d.out_stride_h = ov.stride_t, ov.stride_c, ov.stride_h
    tables = ((C.c_int32 * max(Tk, 1))(*key_frame), (C.c_int32 * max(n, 1))(*frames), (C.c_int32 * max(2 * n, 1))(*[v for s in slots for v in s]),
              (C.c_float * max(2 * n, 1))(*[v for w in weights for v in w]))   # host arrays: the entry reads them before it returns
    d.key_frame, d.frame, d.slot, d.weight = tables
    d.n, d.T, d.Tk, d.H, d.W, d.mode, d.sigma = n, T, Tk, H, W, _lib.KEYFILL_MODES.index(mode), sigma
    check(lib.insv2v_keyframe_fill(_byref(d), _stream()), "insv2v_keyframe_fill")
    return out, (None if conf is False else conf)


# ----------------------------------------------------------------------------- shaping a mask (insv2v/mask_shape.py)
def mask_shape_plan(grow, feather):
    """insv2v_mask_shape_plan: the search radius, FAR and the four integer thresholds of (grow, feather) as a dict; launches nothing."""
    p = _lib.MaskShapePlan()
    check(_lib.load().insv2v_mask_shape_plan(grow, feather, _byref(p)), "insv2v_mask_shape_plan")
    return {n: getattr(p, n) for n, _ in p._fields_ if n != "rc"}


def mask_shape(mask, *, grow=0.0, feather=0.0, threshold=0.5, profile="smooth", return_d2=False, out=None, workspace=None):
    """insv2v_mask_shape (tests/mask_shape_ref.py is the definition): ``mask`` fp32 [T,H,W] -> (shaped, support)
    fp32 [T,H,W], and with ``return_d2`` also (d2_out, d2_in) int32 [T,H,W], the squared distances to the nearest inside / outside
    pixel.  ``out``: those tensors preallocated (a 2- or 4-tuple); ``workspace``: a contiguous uint8 tensor of at least
    insv2v_mask_shape_workspace_bytes(T,H,W) bytes (default: allocated here)."""
    lib = _lib.load()
    _req(mask, torch.float32, "mask_shape.mask")
    if mask.dim() != 3 or not mask.is_contiguous():
        raise _lib.HipKernelError(f"mask_shape: mask {tuple(mask.shape)} must be a contiguous [T,H,W]")
    if profile not in _lib.MASK_PROFILES:
        raise ValueError(f"mask_shape: profile {profile!r} is neither 'linear' nor 'smooth'")
    T, H, W = mask.shape
    if out is None:
        out = tuple(torch.empty_like(mask) for _ in range(2))
        if return_d2:
            out += tuple(torch.empty(mask.shape, device=mask.device, dtype=torch.int32) for _ in range(2))
    if len(out) != (4 if return_d2 else 2):
        raise _lib.HipKernelError(f"mask_shape: out must hold {4 if return_d2 else 2} tensors")
    for i, t in enumerate(out):
        _plain(t, (T, H, W), f"mask_shape.out[{i}]", torch.float32 if i < 2 else torch.int32)
    nbytes = lib.insv2v_mask_shape_workspace_bytes(T, H, W)
    if nbytes <= 0:
        raise _lib.HipKernelError(f"mask_shape: no workspace size for mask {tuple(mask.shape)}")
    if workspace is None:
        workspace = torch.empty(nbytes, device=mask.device, dtype=torch.uint8)
    else:
        _req(workspace, torch.uint8, "mask_shape.workspace")
        if not workspace.is_contiguous():
            raise _lib.HipKernelError("mask_shape: the workspace must be contiguous")
    d = _lib.MaskShapeDesc()
    d.m, d.shaped, d.support = mask.data_ptr() or None, out[0].data_ptr() or None, out[1].data_ptr() or None
    d.d2_out, d.d2_in = (out[2].data_ptr() or None, out[3].data_ptr() or None) if return_d2 else (None, None)
    d.workspace, d.workspace_bytes = workspace.data_ptr() or None, workspace.numel()
    d.T, d.H, d.W, d.threshold, d.grow, d.feather, d.profile = T, H, W, threshold, grow, feather, _lib.MASK_PROFILES.index(profile)
    check(lib.insv2v_mask_shape(_byref(d), _stream()), "insv2v_mask_shape")
    return tuple(out)


# ----------------------------------------------------------------------------- editing a region at full resolution (insv2v/region.py)
def _region_view(t, name):
    """An fp32 CUDA [n,C,H,W] tensor, any view whose rows are contiguous (a broadcast frame or channel has stride 0)."""
    _req(t, torch.float32, name)
    if t.dim() != 4 or (t.shape[3] > 1 and t.stride(3) != 1):
        raise _lib.HipKernelError(f"{name}: {tuple(t.shape)} (strides {t.stride()}) must be [n,C,H,W] with contiguous rows")
    return tuple(t.shape)


def mask_bbox(mask, *, threshold=0.5, out=None):
    """insv2v_mask_bbox (tests/region_ref.py is the definition): ``mask`` fp32 [T,H,W], any view with contiguous
    rows (a [1,H,W] mask expanded to T frames has frame stride 0) -> int32 [T + 1, 4] on the device: per frame and, in the last row,
    over all frames the half-open box (x0, y0, x1, y1) of ``mask > threshold``; (W, H, 0, 0) where there is none."""
    lib = _lib.load()
    _req(mask, torch.float32, "mask_bbox.mask")
    if mask.dim() != 3 or (mask.shape[2] > 1 and mask.stride(2) != 1):
        raise _lib.HipKernelError(f"mask_bbox: mask {tuple(mask.shape)} (strides {mask.stride()}) must be [T,H,W] with contiguous rows")
    T, H, W = mask.shape
    if out is None:
        out = torch.empty((T + 1, 4), device=mask.device, dtype=torch.int32)
    _plain(out, (T + 1, 4), "mask_bbox.out", torch.int32)
    check(lib.insv2v_mask_bbox(mask.data_ptr() or None, mask.stride(0), mask.stride(1), T, H, W, threshold, out.data_ptr() or None, _stream()),
          "insv2v_mask_bbox")
    return out


def region_resample(src, box, size, *, mode="bicubic", clamp=None, out=None):
    """insv2v_region_resample: ``src`` fp32 [n,C,H,W] (any view with contiguous rows), ``box`` (x0, y0, x1, y1) inside the frame,
    ``size`` (w, h) -> fp32 [n,C,h,w]: the box resampled with the antialiased ``mode`` ("bicubic" / "bilinear") of
    ``torch.nn.functional.interpolate``, taps clipped at the box; ``clamp=(lo, hi)`` clamps the result."""
    lib = _lib.load()
    n, Cn, H, W = _region_view(src, "region_resample.src")
    if mode not in _lib.REGION_FILTERS:
        raise ValueError(f"region_resample: mode {mode!r} is neither 'bicubic' nor 'bilinear'")
    w, h = (int(v) for v in size)
    if out is None:
        out = torch.empty((n, Cn, max(h, 0), max(w, 0)), device=src.device, dtype=torch.float32)
    _plain(out, (n, Cn, h, w), "region_resample.out")
    d = _lib.RegionResampleDesc()
    d.src, d.dst = src.data_ptr() or None, out.data_ptr() or None
    d.src_stride_n, d.src_stride_c, d.src_stride_h = src.stride(0), src.stride(1), src.stride(2)
    d.n, d.C, d.H, d.W, d.h, d.w = n, Cn, H, W, h, w
    d.x0, d.y0, d.x1, d.y1 = (int(v) for v in box)
    d.filter, d.clamp = _lib.REGION_FILTERS.index(mode), int(clamp is not None)
    d.clamp_lo, d.clamp_hi = clamp if clamp is not None else (0.0, 0.0)
    check(lib.insv2v_region_resample(_byref(d), _stream()), "insv2v_region_resample")
    return out


def region_paste(out, edit_w, down_src, box, *, mode="residual", blend=8, mask_w=None):
    """insv2v_region_paste, IN PLACE: ``out`` fp32 [n,C,H,W] (any view with contiguous rows) holds the source; its ``box`` takes the
    working-resolution edit ``edit_w`` [n,C,h,w]: ``mode="residual"`` adds ``edit_w - down_src`` resampled to the box, ``"replace"``
    blends the resampled ``edit_w`` in under ``mask_w`` ([n,h,w], or [1,h,w] for every frame, or None: ones), each under the ramp of
    ``blend`` pixels at the box edges that are not frame borders.  Returns ``out``."""
    lib = _lib.load()
    n, Cn, H, W = _region_view(out, "region_paste.out")
    if mode not in _lib.REGION_MODES:
        raise ValueError(f"region_paste: mode {mode!r} is neither 'residual' nor 'replace'")
    _req(edit_w, torch.float32, "region_paste.edit_w")
    if edit_w.dim() != 4 or tuple(edit_w.shape[:2]) != (n, Cn) or not edit_w.is_contiguous():
        raise _lib.HipKernelError(f"region_paste: edit_w {tuple(edit_w.shape)} must be a contiguous [{n},{Cn},h,w]")
    h, w = edit_w.shape[2:]
    d = _lib.RegionPasteDesc()
    if mode == "residual":
        _plain(down_src, (n, Cn, h, w), "region_paste.down_src")
        d.down = down_src.data_ptr() or None
    elif mask_w is not None:
        _req(mask_w, torch.float32, "region_paste.mask_w")
        if mask_w.dim() != 3 or mask_w.shape[0] not in (1, n) or tuple(mask_w.shape[1:]) != (h, w) or not mask_w.is_contiguous():
            raise _lib.HipKernelError(f"region_paste: mask_w {tuple(mask_w.shape)} must be a contiguous [{n},{h},{w}] or [1,{h},{w}]")
        d.mask, d.mask_stride_n = mask_w.data_ptr() or None, (h * w if mask_w.shape[0] == n and n > 1 else 0)
    d.edit, d.out = edit_w.data_ptr() or None, out.data_ptr() or None
    d.out_stride_n, d.out_stride_c, d.out_stride_h = out.stride(0), out.stride(1), out.stride(2)
    d.n, d.C, d.H, d.W, d.h, d.w = n, Cn, H, W, h, w
    d.x0, d.y0, d.x1, d.y1 = (int(v) for v in box)
    d.mode, d.blend = _lib.REGION_MODES.index(mode), float(blend)
    check(lib.insv2v_region_paste(_byref(d), _stream()), "insv2v_region_paste")
    return out


def _track_boxes(boxes, n, name):
    """``boxes``: a sequence of n 4-tuples or an [n,4] float64 CPU tensor -> a ctypes array of n x 4 doubles (the entries read it on the
    host, before they return)."""
    if torch.is_tensor(boxes):
        if boxes.is_cuda or boxes.dtype != torch.float64 or boxes.dim() != 2 or boxes.shape[1] != 4:
            raise _lib.HipKernelError(f"{name}: boxes {tuple(boxes.shape)} ({boxes.dtype}, {boxes.device}) must be an [n,4] float64 CPU tensor")
        boxes = boxes.tolist()
    rows = [tuple(float(v) for v in b) for b in boxes]
    if len(rows) != n or any(len(b) != 4 for b in rows):
        raise _lib.HipKernelError(f"{name}: {len(rows)} boxes for {n} frames: one (x0, y0, x1, y1) per frame")
    return (C.c_double * (4 * n))(*[v for b in rows for v in b])


def region_resample_track(src, boxes, size, *, mode="bicubic", clamp=None, out=None):
    """insv2v_region_resample_track: ``region_resample`` with one real-valued box per frame - ``boxes``, n
    4-tuples (x0, y0, x1, y1) or an [n,4] float64 CPU tensor.  Frame i of ``src`` [n,C,H,W] is resampled from its own box; the taps are
    clipped at the box's cover [floor(x0), ceil(x1)) x [floor(y0), ceil(y1))."""
    lib = _lib.load()
    n, Cn, H, W = _region_view(src, "region_resample_track.src")
    if mode not in _lib.REGION_FILTERS:
        raise ValueError(f"region_resample_track: mode {mode!r} is neither 'bicubic' nor 'bilinear'")
    w, h = (int(v) for v in size)
    arr = _track_boxes(boxes, n, "region_resample_track")
    if out is None:
        out = torch.empty((n, Cn, max(h, 0), max(w, 0)), device=src.device, dtype=torch.float32)
    _plain(out, (n, Cn, h, w), "region_resample_track.out")
    d = _lib.RegionResampleTrackDesc()
    d.src, d.dst, d.boxes = src.data_ptr() or None, out.data_ptr() or None, C.cast(arr, C.c_void_p)
    d.src_stride_n, d.src_stride_c, d.src_stride_h = src.stride(0), src.stride(1), src.stride(2)
    d.n, d.C, d.H, d.W, d.h, d.w = n, Cn, H, W, h, w
    d.filter, d.clamp = _lib.REGION_FILTERS.index(mode), int(clamp is not None)
    d.clamp_lo, d.clamp_hi = clamp if clamp is not None else (0.0, 0.0)
    check(lib.insv2v_region_resample_track(_byref(d), _stream()), "insv2v_region_resample_track")
    return out


def region_paste_track(out, edit_w, down_src, boxes, *, mode="residual", blend=8, mask_w=None):
    """insv2v_region_paste_track, IN PLACE: ``region_paste`` with one real-valued box per frame (``boxes`` as for
    ``region_resample_track``).  Frame i of ``out`` [n,C,H,W], which holds the source, takes the edit in its own box; only the box's
    cover is written, under a ramp measured from the box's real edges.  Returns ``out``."""
    lib = _lib.load()
    n, Cn, H, W = _region_view(out, "region_paste_track.out")
    if mode not in _lib.REGION_MODES:
        raise ValueError(f"region_paste_track: mode {mode!r} is neither 'residual' nor 'replace'")
    _req(edit_w, torch.float32, "region_paste_track.edit_w")
    if edit_w.dim() != 4 or tuple(edit_w.shape[:2]) != (n, Cn) or not edit_w.is_contiguous():
        raise _lib.HipKernelError(f"region_paste_track: edit_w {tuple(edit_w.shape)} must be a contiguous [{n},{Cn},h,w]")
    h, w = edit_w.shape[2:]
    arr = _track_boxes(boxes, n, "region_paste_track")
    d = _lib.RegionPasteTrackDesc()
    if mode == "residual":
        _plain(down_src, (n, Cn, h, w), "region_paste_track.down_src")
        d.down = down_src.data_ptr() or None
    elif mask_w is not None:
        _req(mask_w, torch.float32, "region_paste_track.mask_w")
        if mask_w.dim() != 3 or mask_w.shape[0] not in (1, n) or tuple(mask_w.shape[1:]) != (h, w) or not mask_w.is_contiguous():
            raise _lib.HipKernelError(f"region_paste_track: mask_w {tuple(mask_w.shape)} must be a contiguous [{n},{h},{w}] or [1,{h},{w}]")
        d.mask, d.mask_stride_n = mask_w.data_ptr() or None, (h * w if mask_w.shape[0] == n and n > 1 else 0)
    d.edit, d.out, d.boxes = edit_w.data_ptr() or None, out.data_ptr() or None, C.cast(arr, C.c_void_p)
    d.out_stride_n, d.out_stride_c, d.out_stride_h = out.stride(0), out.stride(1), out.stride(2)
    d.n, d.C, d.H, d.W, d.h, d.w = n, Cn, H, W, h, w
    d.mode, d.blend = _lib.REGION_MODES.index(mode), float(blend)
    check(lib.insv2v_region_paste_track(_byref(d), _stream()), "insv2v_region_paste_track")
    return out
