"""Tensor-level wrappers over the C ABI (one function per entry point of include/drakegpt_hip.h).

PyTorch is plumbing here: it owns device memory (caching allocator) and the stream; every
function extracts raw device pointers, enqueues the HIP kernel on torch's CURRENT stream and
returns (so the calls can be captured into a hipGraph via torch.cuda.graph).  Arguments are
validated on the host before a launch -- a kernel that faults can reset the GPU.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import Optional

import torch

from . import _lib
from ._lib import DG_BF16, DG_F32, DG_F32X3, DG_FP8_E4M3, DG_FP8_E5M2, GemmNtArgs, check, lib

Tensor = torch.Tensor

_DT = {torch.float32: DG_F32, torch.bfloat16: DG_BF16, torch.float8_e4m3fn: DG_FP8_E4M3, torch.float8_e5m2: DG_FP8_E5M2}
FP8_DTYPES = (torch.float8_e4m3fn, torch.float8_e5m2)
FP8_AMAX_PARTS = 256            # DG_FP8_AMAX_PARTS
ATTN_FP8_HIST = 3 * 64 * 32     # DG_ATTN_FP8_HIST


def dt_code(dtype: torch.dtype) -> int:
    try:
        return _DT[dtype]
    except KeyError:
        raise TypeError(f"drakegpt_amd: unsupported dtype {dtype} (float32 / bfloat16 / OCP float8 only)") from None


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _chk(t: Tensor, name: str, dtype=None, contiguous: bool = True) -> None:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"drakegpt_amd: {name} must be a tensor on the GPU (got {getattr(t, 'device', type(t))}); "
                           "the HIP path has no CPU fallback")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"drakegpt_amd: {name} must be {dtype}, got {t.dtype}")
    if contiguous and not t.is_contiguous():
        raise RuntimeError(f"drakegpt_amd: {name} must be contiguous")


def _ld(t: Tensor) -> int:
    """leading dimension (elements) of a 2-D row-major view with unit column stride"""
    if t.dim() != 2 or t.stride(1) != 1:
        raise RuntimeError("drakegpt_amd: expected a 2-D tensor with unit column stride")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1])


def check_ids(ids: Tensor, n: int, what: str, allow: Optional[int] = None) -> None:
    """raise IndexError unless 0 <= ids < n (or ids == allow: the targets' ignore_index) -- what nn.Embedding / F.cross_entropy do in the reference (ref: src/model.py:595,
    606).  The kernels clamp ids so that a bad one can never fault the GPU, which would otherwise turn a tokenizer / vocabulary
    mismatch into a plausible loss on aliased ids.  One device round trip: call it where ids ENTER (module forward, set_corpus,
    set_batch), never inside a captured step."""
    if ids.numel() == 0:
        return
    if allow is not None and not 0 <= allow < n:
        ids = ids[ids != allow]
        if ids.numel() == 0:
            return
    lo, hi = torch.aminmax(ids)
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi >= n:
        raise IndexError(f"index out of range in self: {what} holds ids in [{lo}, {hi}], valid range is [0, {n})")


# ------------------------------------------------------------------------------------------
def new_rng_state(seed: int, device, step: int = 0) -> Tensor:
    """device uint32[4] = {seed_lo, seed_hi, step, 0} (stored as int32 bit patterns)."""
    vals = [seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, step & 0xFFFFFFFF, 0]
    vals = [v - (1 << 32) if v >= (1 << 31) else v for v in vals]
    return torch.tensor(vals, dtype=torch.int32, device=device)


def state_advance(rng_state: Tensor) -> None:
    _chk(rng_state, "rng_state", torch.int32)
    check(lib.dg_state_advance(_p(rng_state), _stream()), "dg_state_advance")


def batch_gather(corpus: Tensor, offsets: Tensor, T: int, x: Optional[Tensor] = None, y: Optional[Tensor] = None):
    _chk(corpus, "corpus", torch.int64)
    _chk(offsets, "offsets", torch.int64)
    B = offsets.numel()
    if x is None:
        x = torch.empty((B, T), dtype=torch.int64, device=corpus.device)
    if y is None:
        y = torch.empty((B, T), dtype=torch.int64, device=corpus.device)
    check(lib.dg_batch_gather(_p(corpus), corpus.numel(), _p(offsets), _p(x), _p(y), B, T, _stream()), "dg_batch_gather")
    return x, y


def embed_fwd(idx: Tensor, tok: Tensor, pos: Optional[Tensor], out: Optional[Tensor] = None,
              onehot: Optional[Tensor] = None) -> Tensor:
    """x = tok[idx] + pos; `onehot` (bf16 [B*T, >= V]) additionally receives one-hot rows of idx"""
    _chk(idx, "idx", torch.int64)
    _chk(tok, "tok", torch.float32)
    B, T = idx.shape
    V, Cd = tok.shape
    if pos is not None:
        _chk(pos, "pos", torch.float32)
        if T > pos.shape[0]:
            raise IndexError(f"index out of range in self: sequence length {T} exceeds context_length {pos.shape[0]}")
    if out is None:
        out = torch.empty((B, T, Cd), dtype=torch.float32, device=idx.device)
    if onehot is not None:
        _chk(onehot, "onehot", torch.bfloat16, contiguous=False)
    check(lib.dg_embed_fwd(_p(idx), _p(tok), _p(pos), _p(out), B, T, Cd, V, _p(onehot), _ld(onehot) if onehot is not None else 0,
                           _stream()), "dg_embed_fwd")
    return out


def batch_embed_fwd(corpus: Tensor, offsets: Tensor, step_state: Optional[Tensor], ctl: Optional[Tensor], x_ids: Tensor, y_ids: Tensor,
                    tok: Tensor, pos: Optional[Tensor], onehot: Optional[Tensor] = None) -> Tensor:
    """get_batch + embedding in one launch: gathers row (step - ctl[0]) of the staged offset block [n_rows, B] from the resident
    corpus, writes the ids / targets into x_ids / y_ids [B, T] and returns x = tok[ids] + pos  [B, T, C]"""
    _chk(corpus, "corpus", torch.int64)
    _chk(offsets, "offsets", torch.int64)
    _chk(x_ids, "x_ids", torch.int64)
    _chk(y_ids, "y_ids", torch.int64)
    _chk(tok, "tok", torch.float32)
    B, T = x_ids.shape
    V, Cd = tok.shape
    if offsets.dim() != 2 or offsets.shape[1] != B or y_ids.shape != x_ids.shape:
        raise ValueError("batch_embed_fwd: offsets must be [n_rows, B] and y_ids shaped like x_ids")
    if (ctl is None) != (step_state is None):
        raise ValueError("batch_embed_fwd: ctl and step_state go together")
    if pos is not None:
        _chk(pos, "pos", torch.float32)
        if T > pos.shape[0]:
            raise IndexError(f"index out of range in self: sequence length {T} exceeds context_length {pos.shape[0]}")
    out = torch.empty((B, T, Cd), dtype=torch.float32, device=tok.device)
    if onehot is not None:
        _chk(onehot, "onehot", torch.bfloat16, contiguous=False)
    check(lib.dg_batch_embed_fwd(_p(corpus), corpus.numel(), _p(offsets), _p(step_state), _p(ctl), _p(x_ids), _p(y_ids), _p(tok), _p(pos),
                                 _p(out), B, T, Cd, V, _p(onehot), _ld(onehot) if onehot is not None else 0, _stream()), "dg_batch_embed_fwd")
    return out


def embed_bwd(idx: Tensor, dx: Tensor, dtok: Optional[Tensor], dpos: Optional[Tensor], V: Optional[int] = None) -> None:
    _chk(idx, "idx", torch.int64)
    _chk(dx, "dx")                         # fp32, or the engine's bf16 gradient stream
    B, T = idx.shape
    if dtok is not None:
        _chk(dtok, "dtok", torch.float32)
        V, Cd = dtok.shape
    else:
        Cd = dx.shape[-1]
    if dpos is not None:
        _chk(dpos, "dpos", torch.float32)
        if dpos.shape[0] != T:
            raise RuntimeError("dpos must be the [T, C] slice of the position gradient")
    check(lib.dg_embed_bwd(_p(idx), _p(dx), dt_code(dx.dtype), _p(dtok), _p(dpos), B, T, Cd, V, _stream()), "dg_embed_bwd")


def layernorm_fwd(x: Tensor, gamma: Tensor, beta: Tensor, out_dtype: torch.dtype, eps: float = 1e-5):
    _chk(x, "x", torch.float32)
    _chk(gamma, "gamma", torch.float32)
    _chk(beta, "beta", torch.float32)
    Cd = x.shape[-1]
    M = x.numel() // Cd
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    mean = torch.empty((M,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((M,), dtype=torch.float32, device=x.device)
    check(lib.dg_layernorm_fwd(_p(x), _p(gamma), _p(beta), _p(y), dt_code(out_dtype), _p(mean), _p(rstd), M, Cd, eps, _stream()),
          "dg_layernorm_fwd")
    return y, mean, rstd


def layernorm_fwd_fp8_parts(M: int) -> int:
    """partial maxima per history slot of layernorm_fwd_fp8 (one per workgroup of its launch)"""
    return int(lib.dg_layernorm_fwd_fp8_parts(int(M)))


def layernorm_fwd_fp8(x: Tensor, gamma: Tensor, beta: Tensor, parts2: Tensor, step_state: Tensor, want_bf16: bool = True, eps: float = 1e-5):
    """LayerNorm whose output leaves as e4m3 with delayed scaling (parts2: fp32 [2 * layernorm_fwd_fp8_parts(M)], this call site's
    history).  Returns (y bf16 -- unwritten and marked dg_unwritten when want_bf16 is False --, mean, rstd, q8, scale_inv [1])."""
    _chk(x, "x", torch.float32)
    _chk(gamma, "gamma", torch.float32)
    _chk(beta, "beta", torch.float32)
    _chk(parts2, "parts2", torch.float32)
    _chk(step_state, "step_state", torch.int32)
    Cd = x.shape[-1]
    M = x.numel() // Cd
    n = layernorm_fwd_fp8_parts(M)
    if parts2.numel() != 2 * n:
        raise RuntimeError(f"layernorm_fwd_fp8: parts2 must hold 2 x {n} floats")
    y = torch.empty(x.shape, dtype=torch.bfloat16, device=x.device)
    q8 = torch.empty(x.shape, dtype=torch.float8_e4m3fn, device=x.device)
    mean = torch.empty((M,), dtype=torch.float32, device=x.device)
    rstd = torch.empty((M,), dtype=torch.float32, device=x.device)
    sinv = torch.empty((1,), dtype=torch.float32, device=x.device)
    check(lib.dg_layernorm_fwd_fp8(_p(x), _p(gamma), _p(beta), _p(y) if want_bf16 else None, _p(q8), _p(mean), _p(rstd), M, Cd, eps, _p(parts2), n,
                                   _p(step_state), _p(sinv), _stream()), "dg_layernorm_fwd_fp8")
    if not want_bf16:
        y.dg_unwritten = True
    return y, mean, rstd, q8, sinv


def layernorm_bwd(dy: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor, dresid: Optional[Tensor],
                  dgamma_part: Tensor, dbeta_part: Tensor, part_stride: int, n_partials: int,
                  dx: Optional[Tensor] = None) -> Tensor:
    _chk(dy, "dy")                        # fp32, or bf16 straight from a dX GEMM
    _chk(x, "x", torch.float32)
    if dresid is not None:
        _chk(dresid, "dresid", torch.float32)
    Cd = x.shape[-1]
    M = x.numel() // Cd
    if dx is None:
        dx = torch.empty_like(x)
    check(lib.dg_layernorm_bwd(_p(dy), dt_code(dy.dtype), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dresid), _p(dx), _p(dgamma_part), _p(dbeta_part),
                               part_stride, n_partials, M, Cd, _stream()), "dg_layernorm_bwd")
    return dx


def layernorm_bwd_fused(dy: Tensor, x: Tensor, gamma: Tensor, mean: Tensor, rstd: Tensor, dresid: Optional[Tensor],
                        dgamma_part: Tensor, dbeta_part: Tensor, part_stride: int, n_partials: int,
                        g_dtype: torch.dtype, p: float, rng_state: Optional[Tensor], site: int, gbias_part: Optional[Tensor],
                        stream_dtype: torch.dtype = torch.float32, fp8_out=None, fp8_out_only: bool = False):
    """layernorm_bwd that also emits g = dropout_bwd(dx) in g_dtype and its column-sum partials; returns (dx, g).
    stream_dtype: type of dresid (in) and dx (out), fp32 or bf16 (the engine's bf16 gradient stream: bf16 dy and g only).
    fp8_out = (parts2 fp32 [2 * FP8_AMAX_PARTS], step_state): g (bf16) also leaves as e5m2 with delayed scaling -- the operand of
    the fp8 dX GEMM that runs next; n_partials must be FP8_AMAX_PARTS.  Returns (dx, g, g8, scale_inv [1]) then."""
    _chk(dy, "dy")
    _chk(x, "x", torch.float32)
    if dresid is not None:
        _chk(dresid, "dresid", stream_dtype)
    Cd = x.shape[-1]
    M = x.numel() // Cd
    dx = torch.empty(x.shape, dtype=stream_dtype, device=x.device)
    g = torch.empty(x.shape, dtype=g_dtype, device=x.device)
    if fp8_out is not None:
        parts2, step_state = fp8_out
        _chk(parts2, "fp8_out parts2", torch.float32)
        _chk(step_state, "fp8_out step_state", torch.int32)
        if g_dtype != torch.bfloat16 or parts2.numel() != 2 * FP8_AMAX_PARTS or n_partials != FP8_AMAX_PARTS:
            raise RuntimeError("layernorm_bwd_fused: fp8_out needs a bf16 g, a [2 * FP8_AMAX_PARTS] history and n_partials == FP8_AMAX_PARTS")
        g8 = torch.empty(x.shape, dtype=torch.float8_e5m2, device=x.device)
        sinv = torch.empty((1,), dtype=torch.float32, device=x.device)
        check(lib.dg_layernorm_bwd_fused_fp8(_p(dy), dt_code(dy.dtype), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dresid), _p(dx), dt_code(stream_dtype),
                                             _p(dgamma_part), _p(dbeta_part), part_stride, n_partials, M, Cd, _p(g), float(p),
                                             _p(rng_state) if p > 0.0 else None, site, _p(gbias_part), _p(g8), _p(parts2), _p(step_state), _p(sinv),
                                             1 if fp8_out_only else 0, _stream()), "dg_layernorm_bwd_fused_fp8")
        if fp8_out_only:
            g.dg_unwritten = True           # (its consumers read g8)
        return dx, g, g8, sinv
    check(lib.dg_layernorm_bwd_fused(_p(dy), dt_code(dy.dtype), _p(x), _p(gamma), _p(mean), _p(rstd), _p(dresid), _p(dx), dt_code(stream_dtype), _p(dgamma_part),
                                     _p(dbeta_part), part_stride, n_partials, M, Cd, _p(g), dt_code(g_dtype), float(p),
                                     _p(rng_state) if p > 0.0 else None, site, _p(gbias_part), _stream()), "dg_layernorm_bwd_fused")
    return dx, g


def layernorm_bwd_fused_supported(C: int) -> bool:
    return C % 4 == 0 and C <= 1024


def gemm_nt_args(A: Tensor, Bm: Tensor, out_dtype: torch.dtype, *, N: Optional[int] = None, K: Optional[int] = None,
                 bias: Optional[Tensor] = None, relu: bool = False, relu_mask: Optional[Tensor] = None,
                 residual: Optional[Tensor] = None, dropout_p: float = 0.0, rng_state: Optional[Tensor] = None,
                 site: int = 0, out: Optional[Tensor] = None, sign_bits_out: Optional[Tensor] = None,
                 sign_bits: Optional[Tensor] = None, colsum_part: Optional[Tensor] = None,
                 scale_a: Optional[Tensor] = None, scale_b: Optional[Tensor] = None, fp8_out=None, fp8_out_only: bool = False,
                 split: bool = False):
    """out[M,N] = epilogue(A[M,K] @ Bm[N,K]^T).  A/Bm may carry padding columns beyond K (ld > K).
    split: fp32 A / Bm / relu_mask contracted as split bf16 (hi.hi + hi.lo + lo.hi, precision "bf16x3"); fp32 output.
    fp8_out_only: with fp8_out, do not write `out` (nobody reads the bf16 form); the returned tensor is marked dg_unwritten.
    fp8_out: (q8 [M, N] float8_e4m3fn -- float8_e5m2 in the dX direction --, parts2 fp32 [2 * FP8_AMAX_PARTS], step_state, scale_inv fp32 [1]) -- the epilogue also
    writes the output as e4m3 with delayed scaling (what fp8_quantize_delayed would make of it); only where
    gemm_nt_fp8_out_supported(M, N, K).
    fp8: A float8_e4m3fn (activations) or float8_e5m2 (gradients), Bm float8_e4m3fn, scale_a / scale_b the device scalars
    fp8_quantize returned (out = epilogue(scale_a * scale_b * A @ Bm^T)); K % 128 == 0.
    sign_bits_out / sign_bits: opaque uint8 buffer (new_sign_bits) holding one bit per element, out > 0.
    colsum_part: fp32 [gemm_nt_colsum_rows(...), N] (rows may be strided): partial rows of the column sums of out.

    This is the argument builder: every check of a gemm_nt call and the filled dg_gemm_nt_args; returns (args, out) and launches
    nothing (gemm_nt makes the call; the tests hand the struct to the library's launch plan)."""
    _chk(A, "A", contiguous=False)
    _chk(Bm, "B", contiguous=False)
    fp8 = A.dtype in FP8_DTYPES
    if split and (A.dtype != torch.float32 or Bm.dtype != torch.float32 or out_dtype != torch.float32
                  or (out is not None and out.dtype != torch.float32)):
        raise TypeError(f"gemm_nt: split=True needs fp32 operands and an fp32 output (got {A.dtype}, {Bm.dtype} -> {out_dtype})")
    if fp8:
        if Bm.dtype != torch.float8_e4m3fn or scale_a is None or scale_b is None:
            raise TypeError("gemm_nt: fp8 operands need a float8_e4m3fn B operand and both dequantisation scales")
        _chk(scale_a, "scale_a", torch.float32)
        _chk(scale_b, "scale_b", torch.float32)
    elif A.dtype != Bm.dtype:
        raise TypeError(f"gemm_nt: operand dtypes differ ({A.dtype} vs {Bm.dtype})")
    M = A.shape[0]
    K = A.shape[1] if K is None else K
    N = Bm.shape[0] if N is None else N
    if out is None:
        out = torch.empty((M, N), dtype=out_dtype, device=A.device)
    a = GemmNtArgs()
    a.A, a.lda = _p(A), _ld(A)
    a.B, a.ldb = _p(Bm), _ld(Bm)
    a.C, a.ldc = _p(out), _ld(out)
    a.M, a.N, a.K = M, N, K
    a.in_dtype, a.out_dtype = (DG_F32X3 if split else dt_code(A.dtype)), dt_code(out.dtype)
    if fp8:
        a.b_dtype, a.scale_a, a.scale_b = dt_code(Bm.dtype), _p(scale_a), _p(scale_b)
    if bias is not None:
        _chk(bias, "bias", torch.float32)
        if bias.numel() != N:
            raise RuntimeError("gemm_nt: bias size mismatch")
    a.bias = _p(bias)
    a.relu = 1 if relu else 0
    if relu_mask is not None:
        if fp8:
            raise TypeError("gemm_nt: the tensor-valued relu_mask is not offered for fp8 operands (use sign_bits)")
        _chk(relu_mask, "relu_mask", A.dtype, contiguous=False)
        a.relu_mask, a.ldmask = _p(relu_mask), _ld(relu_mask)
    if residual is not None:
        _chk(residual, "residual", torch.float32, contiguous=False)
        a.residual, a.ldr = _p(residual), _ld(residual)
    a.dropout_p = float(dropout_p)
    a.rng_state = _p(rng_state) if dropout_p > 0.0 else None
    a.site = site
    for name, t in (("sign_bits_out", sign_bits_out), ("sign_bits", sign_bits)):
        if t is not None:
            _chk(t, name, torch.uint8)
            setattr(a, name, _p(t))
            a.sign_bits_bytes = t.numel()
    if colsum_part is not None:
        _chk(colsum_part, "colsum_part", torch.float32, contiguous=False)
        if colsum_part.shape[1] < N:
            raise RuntimeError("gemm_nt: colsum_part must have N columns")
        a.colsum_part, a.colsum_ld, a.colsum_rows = _p(colsum_part), _ld(colsum_part), colsum_part.shape[0]
    if fp8_out is not None:
        q8, parts2, step_state, q_scale_inv = fp8_out
        _chk(q8, "fp8_out", torch.float8_e5m2 if A.dtype == torch.float8_e5m2 else torch.float8_e4m3fn, contiguous=False)
        _chk(parts2, "fp8_out parts2", torch.float32)
        _chk(q_scale_inv, "fp8_out scale_inv", torch.float32)
        if q8.shape != (M, N) or parts2.numel() < 2 * FP8_AMAX_PARTS:
            raise RuntimeError("gemm_nt: fp8_out must be [M, N] with a [2 * FP8_AMAX_PARTS] history")
        a.fp8_out, a.ld_fp8_out = _p(q8), _ld(q8)
        a.fp8_out_parts2, a.fp8_out_step, a.fp8_out_scale_inv = _p(parts2), _p(step_state), _p(q_scale_inv)
        if fp8_out_only:
            # the bf16 form stays unwritten (the tensor is returned as the carrier of the fp8 copy's attributes only); a consumer
            # that would read it must refuse: dg_unwritten marks it
            a.fp8_out_only = 1
            out.dg_unwritten = True
    elif fp8_out_only:
        raise RuntimeError("gemm_nt: fp8_out_only needs fp8_out")
    return a, out


def gemm_nt(A: Tensor, Bm: Tensor, out_dtype: torch.dtype, **options) -> Tensor:
    """gemm_nt_args(...) and the launch: out[M,N] = epilogue(A[M,K] @ Bm[N,K]^T) on torch's current stream"""
    a, out = gemm_nt_args(A, Bm, out_dtype, **options)
    check(lib.dg_gemm_nt(C.byref(a), _stream()), "dg_gemm_nt")
    return out


def gemm_nt_fp8_out_supported(M: int, N: int, K: int, grad: bool = False) -> bool:
    """can dg_gemm_nt also emit its output as fp8 (fp8_out)?  grad = False: the bias + ReLU + sign-bit form on e4m3 operands
    (e4m3 copy); grad = True: the sign-bit-masked dX form with column sums on e5m2 gradients (e5m2 copy)"""
    a = GemmNtArgs()
    a.M, a.N, a.K = M, N, K
    a.in_dtype, a.out_dtype = dt_code(torch.float8_e5m2 if grad else torch.float8_e4m3fn), dt_code(torch.bfloat16)
    a.ldc = N
    a.C = 16                                   # any non-null, aligned pointer value: the query only looks at which operands are present
    if grad:
        a.sign_bits = a.colsum_part = 16
    else:
        a.bias = a.sign_bits_out = 16
        a.relu = 1
    return bool(lib.dg_gemm_nt_fp8_out_supported(C.byref(a)))


def gemm_nt_sign_bits_supported(dtype: torch.dtype, N: int, K: int, in_dtype: Optional[torch.dtype] = None) -> bool:
    """can dg_gemm_nt emit / consume the one-bit-per-element ReLU mask for this problem?  (dtype: output / activation type;
    in_dtype: operand type when it differs -- the fp8 forms)"""
    a = GemmNtArgs()
    a.M, a.N, a.K = 128, N, K
    a.out_dtype = dt_code(dtype)
    a.in_dtype = dt_code(in_dtype or dtype)
    return bool(lib.dg_gemm_nt_sign_bits_supported(C.byref(a)))


def gemm_nt_colsum_rows(dtype: torch.dtype, M: int, N: int, K: int, in_dtype: Optional[torch.dtype] = None) -> int:
    """partial rows the sign_bits-consuming dg_gemm_nt of this shape writes into colsum_part (0: column sums not offered)"""
    a = GemmNtArgs()
    a.M, a.N, a.K = M, N, K
    a.out_dtype = dt_code(dtype)
    a.in_dtype = dt_code(in_dtype or dtype)
    a.ldc = N
    a.sign_bits = 16        # any non-null, aligned pointer value: the query only looks at which operands are present
    return int(lib.dg_gemm_nt_colsum_rows(C.byref(a)))


def fp8_quantize(x: Tensor, fmt: torch.dtype, seg: Optional[Tensor] = None, n_seg: int = 0, out: Optional[Tensor] = None,
                 scale_inv: Optional[Tensor] = None, amax: Optional[Tensor] = None, reuse_amax: bool = False):
    """per-tensor (per-segment) just-in-time scaling: q = fp8(x * FMAX / amax(x)) and the dequantisation factor amax / FMAX.
    x: contiguous bf16 / fp32, numel % 8 == 0.  seg: int64 device table [n_seg, 2] {first element, count} over x.view(-1)
    (all weight matrices of a step in two launches).  Returns (q with x's shape and dtype `fmt`, scale_inv [n_seg or 1])."""
    _chk(x, "x")
    if fmt not in FP8_DTYPES:
        raise TypeError("fp8_quantize: fmt must be torch.float8_e4m3fn or torch.float8_e5m2")
    ns = n_seg if seg is not None else 1
    if seg is not None:
        _chk(seg, "seg", torch.int64)
    if out is None:
        out = torch.empty(x.shape, dtype=fmt, device=x.device)
    if scale_inv is None:
        scale_inv = torch.empty((ns,), dtype=torch.float32, device=x.device)
    if amax is None:
        amax = torch.empty((ns * FP8_AMAX_PARTS,), dtype=torch.float32, device=x.device)      # partial maxima, reduced by the cast kernel
    n = x.numel()
    if not reuse_amax:          # reuse_amax: `amax` already holds the partial maxima of the same values (W^T after W)
        check(lib.dg_fp8_amax(_p(x), dt_code(x.dtype), n, _p(seg), ns, _p(amax), _stream()), "dg_fp8_amax")
    check(lib.dg_fp8_quantize(_p(x), dt_code(x.dtype), _p(out), dt_code(fmt), n, _p(seg), ns, _p(amax), _p(scale_inv), _stream()),
          "dg_fp8_quantize")
    return out, scale_inv


def fp8_quantize_delayed(x: Tensor, fmt: torch.dtype, parts2: Tensor, rng_state: Tensor):
    """one-pass delayed scaling: scale from the amax this call site recorded one step ago (parts2 [2 * FP8_AMAX_PARTS] fp32, the
    slot chosen by the device-side step word rng_state[2]); records this tensor's amax for the next step.
    Returns (q, scale_inv [1])."""
    _chk(x, "x")
    _chk(parts2, "parts2", torch.float32)
    _chk(rng_state, "rng_state", torch.int32)
    if parts2.numel() != 2 * FP8_AMAX_PARTS:
        raise RuntimeError("fp8_quantize_delayed: parts2 must hold 2 x FP8_AMAX_PARTS floats")
    out = torch.empty(x.shape, dtype=fmt, device=x.device)
    scale_inv = torch.empty((1,), dtype=torch.float32, device=x.device)
    check(lib.dg_fp8_quantize_delayed(_p(x), dt_code(x.dtype), _p(out), dt_code(fmt), x.numel(), _p(parts2), _p(rng_state), _p(scale_inv),
                                      _stream()), "dg_fp8_quantize_delayed")
    return out, scale_inv


def new_sign_bits(M: int, N: int, device) -> Tensor:
    """buffer for gemm_nt(sign_bits_out=...) of an [M, N] output"""
    return torch.empty(int(lib.dg_gemm_nt_sign_bits_bytes(M, N)), dtype=torch.uint8, device=device)


def gemm_tn(A: Tensor, Bm: Tensor, out_part: Tensor, split_stride: int, n_splits: int, P: int, Q: int, ldo: Optional[int] = None,
            split: bool = False) -> None:
    """partials of dW[P,Q] = sum_r A[r,:P]^T B[r,:Q] into out_part (+ s*split_stride).
    split: fp32 operands contracted as split bf16 (precision "bf16x3")."""
    _chk(A, "A", contiguous=False)
    _chk(Bm, "B", contiguous=False)
    _chk(out_part, "out_part", torch.float32, contiguous=False)
    if split and (A.dtype != torch.float32 or Bm.dtype != torch.float32):
        raise TypeError(f"gemm_tn: split=True needs fp32 operands (got {A.dtype}, {Bm.dtype})")
    if A.dtype != Bm.dtype or A.shape[0] != Bm.shape[0]:
        raise RuntimeError("gemm_tn: operand mismatch")
    check(lib.dg_gemm_tn(_p(A), _ld(A), _p(Bm), _ld(Bm), _p(out_part), Q if ldo is None else ldo, split_stride, n_splits,
                         A.shape[0], P, Q, DG_F32X3 if split else dt_code(A.dtype), _stream()), "dg_gemm_tn")


def _tn_problem_array(problems):
    """problems: (A, B, out, P, Q) with bf16 operands, or (A e5m2, B e4m3, out, P, Q, scale_a, scale_b).  Returns (array, dtype code)"""
    from ._lib import TnProblem
    arr = (TnProblem * len(problems))()
    f8 = len(problems[0]) == 7
    for t, pr in zip(arr, problems):
        if (len(pr) == 7) != f8:
            raise RuntimeError("gemm_tn_grouped: bf16 and fp8 problems go into separate calls")
        A, Bm, out, P, Q = pr[:5]
        if f8:
            _chk(A, "A", torch.float8_e5m2, contiguous=False)
            _chk(Bm, "B", torch.float8_e4m3fn, contiguous=False)
            _chk(pr[5], "scale_a", torch.float32)
            _chk(pr[6], "scale_b", torch.float32)
            t.scale_a, t.scale_b = _p(pr[5]), _p(pr[6])
        else:
            _chk(A, "A", torch.bfloat16, contiguous=False)
            _chk(Bm, "B", torch.bfloat16, contiguous=False)
        _chk(out, "out", torch.float32, contiguous=False)
        if A.shape[0] != Bm.shape[0] or out.numel() < P * Q:
            raise RuntimeError("gemm_tn_grouped: operand mismatch")
        t.A, t.lda, t.B, t.ldb, t.out, t.ldo = _p(A), _ld(A), _p(Bm), _ld(Bm), _p(out), Q
        t.R, t.P, t.Q, t.reserved = A.shape[0], P, Q, 0
    return arr, (DG_FP8_E5M2 if f8 else DG_BF16)


def gemm_tn_grouped_workspace(problems, device) -> Tensor:
    """zero-filled split-K workspace for gemm_tn_grouped on these problems (allocate once, pass to every call)"""
    arr, _ = _tn_problem_array(problems)
    return torch.zeros(max(16, int(lib.dg_gemm_tn_grouped_workspace_bytes(arr, len(problems)))), dtype=torch.uint8, device=device)


def gemm_tn_grouped(problems, workspace: Optional[Tensor] = None) -> None:
    """every dW of a backward pass in one launch: problems = [(A [R,>=P], B [R,>=Q], out [P,Q] fp32, P, Q), ...];
    out_i = A_i[:, :P]^T B_i[:, :Q] over all R rows (bf16 operands, R % 64 == 0).  fp8 form: [(A e5m2, B e4m3, out, P, Q,
    scale_a [1], scale_b [1]), ...] with R % 128 == 0: out_i = scale_a * scale_b * A_i^T B_i.  The caller keeps the operands alive.
    `workspace` (gemm_tn_grouped_workspace) lets the kernel split the contraction of every tile in two."""
    arr, code = _tn_problem_array(problems)
    if workspace is not None:
        _chk(workspace, "workspace", torch.uint8)
    check(lib.dg_gemm_tn_grouped(arr, len(problems), code, _p(workspace) if workspace is not None else None,
                                 workspace.numel() if workspace is not None else 0, _stream()), "dg_gemm_tn_grouped")


def reduce_partials(part: Tensor, stride: int, n_partials: int, out: Tensor, n: int) -> None:
    _chk(part, "partials", torch.float32, contiguous=False)
    _chk(out, "out", torch.float32, contiguous=False)
    check(lib.dg_reduce_partials(_p(part), stride, n_partials, _p(out), n, _stream()), "dg_reduce_partials")


def colsum(A: Tensor, part: Tensor, part_stride: int, n_partials: int, N: Optional[int] = None) -> None:
    _chk(A, "A", contiguous=False)
    M = A.shape[0]
    N = A.shape[1] if N is None else N
    check(lib.dg_colsum(_p(A), _ld(A), dt_code(A.dtype), _p(part), part_stride, n_partials, M, N, _stream()), "dg_colsum")


def dropout_bwd_cast(dy: Tensor, out_dtype: Optional[torch.dtype], p: float, rng_state: Optional[Tensor], site: int,
                     relu_mask: Optional[Tensor] = None, colsum_part: Optional[Tensor] = None, part_stride: int = 0,
                     n_partials: int = 0, want_g: bool = True) -> Optional[Tensor]:
    _chk(dy, "dy", contiguous=False)          # fp32, or bf16 (the engine's gradient stream)
    M, N = dy.shape
    g = torch.empty((M, N), dtype=out_dtype, device=dy.device) if want_g else None
    if relu_mask is not None:
        _chk(relu_mask, "relu_mask", torch.float32, contiguous=False)
    check(lib.dg_dropout_bwd_cast(_p(dy), dt_code(dy.dtype), _ld(dy), _p(g), N, dt_code(out_dtype) if want_g else DG_F32, M, N, float(p),
                                  _p(rng_state) if p > 0.0 else None, site,
                                  _p(relu_mask), _ld(relu_mask) if relu_mask is not None else 0,
                                  _p(colsum_part), part_stride, n_partials, _stream()), "dg_dropout_bwd_cast")
    return g


def cast(x: Tensor, out_dtype: torch.dtype, out: Optional[Tensor] = None) -> Tensor:
    _chk(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    check(lib.dg_cast(_p(x), dt_code(x.dtype), _p(out), dt_code(out.dtype), x.numel(), _stream()), "dg_cast")
    return out


def transpose_cast(W: Tensor, out_dtype: torch.dtype, ldo: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """W [R,C] fp32 -> W^T [C, ldo] (ldo >= R, zero padded) in out_dtype."""
    _chk(W, "W", torch.float32, contiguous=False)
    R, Cc = W.shape
    if ldo is None:
        g = 8 if out_dtype == torch.bfloat16 else 4
        ldo = (R + g - 1) // g * g
    if out is None:
        out = torch.empty((Cc, ldo), dtype=out_dtype, device=W.device)
    check(lib.dg_transpose_cast(_p(W), _ld(W), _p(out), ldo, dt_code(out.dtype), R, Cc, _stream()), "dg_transpose_cast")
    return out


def _transpose_table(pairs, device, tile: int) -> tuple:
    """(table, rows, tiles) of a batched transposition in tile x tile tiles: pairs = [(W [R, C], Wt [C, ldo >= R])]"""
    rows, first = [], 0
    for W, Wt in pairs:
        R, Cc = W.shape
        ldo = Wt.shape[1]
        tiles_x, tiles_y = (Cc + tile - 1) // tile, (ldo + tile - 1) // tile
        rows.append([W.data_ptr(), Wt.data_ptr(), _ld(W), ldo, R, Cc, first, tiles_x])
        first += tiles_x * tiles_y
    return torch.tensor(rows, dtype=torch.int64, device=device), len(rows), first


def make_transpose_table(pairs, device) -> tuple:
    """descriptor table for transpose_cast_batched: pairs = [(W [R,C] fp32 or bf16, Wt [C, ldo])]"""
    return _transpose_table(pairs, device, 64)


def make_transpose_u8_table(pairs, device) -> tuple:
    """descriptor table for transpose_u8_batched: pairs = [(W8 [R, C] one-byte elements, Wt8 [C, ldo >= R])]"""
    return _transpose_table(pairs, device, 128)


def transpose_u8_batched(table: Tensor, n_desc: int, total_tiles: int) -> None:
    _chk(table, "table", torch.int64)
    check(lib.dg_transpose_u8_batched(_p(table), n_desc, total_tiles, _stream()), "dg_transpose_u8_batched")


def transpose_cast_batched(table: Tensor, n_desc: int, total_tiles: int, dtype: torch.dtype, in_dtype: torch.dtype = torch.float32) -> None:
    _chk(table, "table", torch.int64)
    check(lib.dg_transpose_cast_batched(_p(table), n_desc, total_tiles, dt_code(in_dtype), dt_code(dtype), _stream()), "dg_transpose_cast_batched")


def attn_fp8_out_supported(B: int, T: int, NH: int, H: int, dtype: torch.dtype) -> bool:
    """can attn_fwd / attn_bwd leave their outputs as fp8 too (fp8_out=...)?"""
    return bool(lib.dg_attn_fp8_out_supported(B, T, NH, H, dt_code(dtype)))


def new_attn_fp8_history(amax: Tensor) -> Tensor:
    """history of an attention fp8 call site (DG_ATTN_FP8_HIST floats: three slots of 64 partial maxima, one 128-byte line each --
    view(3, 64, 32)[s, i, 0]), every word seeded with `amax` (a device scalar)"""
    return amax.detach().float().reshape(1).expand(ATTN_FP8_HIST).contiguous()


def _attn_fp8_arg(fp8_out, shape, fmt: torch.dtype, dev, only8: bool = False):
    """fp8_out = (hist3, step_state) -> (struct, q8, scale_inv)"""
    from ._lib import AttnFp8Out
    hist3, step_state = fp8_out
    _chk(hist3, "hist3", torch.float32)
    if hist3.numel() != ATTN_FP8_HIST:
        raise RuntimeError("attention fp8 history must hold ATTN_FP8_HIST floats (ops.new_attn_fp8_history)")
    q8 = torch.empty(shape, dtype=fmt, device=dev)
    sinv = torch.empty((1,), dtype=torch.float32, device=dev)
    return AttnFp8Out(_p(q8), _p(hist3), _p(step_state), _p(sinv), 1 if only8 else 0), q8, sinv


def doc_starts(ids: Tensor, sep: int, out: Optional[Tensor] = None) -> Tensor:
    """ids int64 [B, T] (rows may be strided) -> int32 [B*T]: starts[b, t] = 1 + the last j < t with ids[b, j] == sep, or 0 -- the
    first key query t may attend to under the document mask (a document ends WITH its separator)."""
    if ids.dim() != 2 or ids.dtype != torch.int64 or not ids.is_cuda or (ids.shape[1] > 1 and ids.stride(1) != 1):
        raise RuntimeError("doc_starts: ids must be a CUDA int64 [B, T] tensor with contiguous rows")
    B, T = ids.shape
    if out is None:
        out = torch.empty(B * T, dtype=torch.int32, device=ids.device)
    else:
        _chk_doc_starts(out, B, T)
    check(lib.dg_doc_starts(_p(ids), ids.stride(0) if B > 1 else T, B, T, int(sep), _p(out), _stream()), "dg_doc_starts")
    return out


def _chk_doc_starts(doc_starts: Tensor, B: int, T: int) -> None:
    _chk(doc_starts, "doc_starts", torch.int32)
    if doc_starts.numel() != B * T:
        raise RuntimeError(f"doc_starts holds {doc_starts.numel()} values, expected B*T = {B * T}")


def _attn_entry(base: str, args: tuple, fp8_arg, doc_starts: Optional[Tensor]) -> None:
    """dg_attn_fwd / dg_attn_bwd; with an fp8 copy their _fp8 form, with document starts their _doc form (fp8 nullable there)"""
    if doc_starts is not None:
        name, tail = base + "_doc", (C.byref(fp8_arg) if fp8_arg is not None else None, _p(doc_starts))
    elif fp8_arg is not None:
        name, tail = base + "_fp8", (C.byref(fp8_arg),)
    else:
        name, tail = base, ()
    check(getattr(lib, name)(*args, *tail, _stream()), name)


def attn_fwd(qkv: Tensor, B: int, T: int, NH: int, H: int, scale: float, p: float, rng_state: Optional[Tensor], site: int,
             keep: bool = False, fp8_out=None, doc_starts: Optional[Tensor] = None):
    """doc_starts (int32 [B*T], ops.doc_starts): document mask -- query i attends to keys doc_starts[b, i] <= j <= i only.
    fp8_out = (hist3, step_state) (precision fp8, attn_fp8_out_supported): the output also as e4m3 with delayed scaling -- the
    attribute `dg_fp8` = (e4m3 copy, scale_inv) travels with it.
    keep=True (training with dropout, a backward pass follows): the forward pass also leaves its dropout keep decisions as
    wave masks (dg_attn_keep_bits_bytes; 128 bytes per unmasked 32 x 32 tile) -- they travel with the output as its attribute
    `dg_keep` and attn_bwd(..., keep_bits=out.dg_keep) selects with them instead of hashing again.  Shapes on the generic
    kernels have no such path (no attribute is set)."""
    _chk(qkv, "qkv")
    if qkv.shape != (B * T, 3 * NH * H):
        raise RuntimeError(f"attn_fwd: qkv shape {tuple(qkv.shape)} != {(B * T, 3 * NH * H)}")
    out = torch.empty((B * T, NH * H), dtype=qkv.dtype, device=qkv.device)
    lse = torch.empty((B, NH, T), dtype=torch.float32, device=qkv.device)
    kb = None
    if keep and p > 0.0 and rng_state is not None:
        n = int(lib.dg_attn_keep_bits_bytes(B, T, NH, H, dt_code(qkv.dtype)))
        if n > 0:
            kb = torch.empty(n, dtype=torch.uint8, device=qkv.device)
    if doc_starts is not None:
        _chk_doc_starts(doc_starts, B, T)
    arg = None
    if fp8_out is not None:
        arg, q8, sinv = _attn_fp8_arg(fp8_out, (B * T, NH * H), torch.float8_e4m3fn, qkv.device)
    _attn_entry("dg_attn_fwd", (_p(qkv), _p(out), _p(lse), B, T, NH, H, float(scale), float(p), _p(rng_state) if p > 0.0 else None,
                                site, dt_code(qkv.dtype), _p(kb), kb.numel() if kb is not None else 0), arg, doc_starts)
    if arg is not None:
        out.dg_fp8 = (q8, sinv)
    if kb is not None:
        out.dg_keep = kb
    return out, lse


def attn_bwd(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, B: int, T: int, NH: int, H: int, scale: float, p: float,
             rng_state: Optional[Tensor], site: int, keep_bits: Optional[Tensor] = None, fp8_out=None, fp8_out_only: bool = False, *,
             tile_scratch: bool = True, doc_starts: Optional[Tensor] = None) -> Tensor:
    """doc_starts: the document mask of the forward pass (attn_fwd); on a shape that takes the MFMA kernels it needs the tile
    scratch (the recompute form of the dK/dV pass has no document variant): ValueError with tile_scratch=False.
    keep_bits: the forward pass's keep masks (attn_fwd(..., keep=True) leaves them as out.dg_keep); default: taken from `out`.
    fp8_out = (hist3, step_state): dqkv also as e5m2 (attribute `dg_fp8` = (e5m2 copy, scale_inv)); fp8_out_only: the bf16 dqkv is
    not written (marked `dg_unwritten`).
    tile_scratch=False: the workspace holds the delta floats only, and the dK/dV pass recomputes the scores instead of reading the
    dQ pass's P | dS tiles (the fp8 output needs the tiles)."""
    _chk(qkv, "qkv")
    if keep_bits is None:
        keep_bits = getattr(out, "dg_keep", None)
    if keep_bits is not None:
        _chk(keep_bits, "keep_bits", torch.uint8)
    _chk(out, "out", qkv.dtype)
    _chk(dout, "dout", qkv.dtype)
    _chk(lse, "lse", torch.float32)
    dqkv = torch.empty_like(qkv)
    nws = lib.dg_attn_bwd_workspace_bytes(B, T, NH, H, dt_code(qkv.dtype)) if tile_scratch else B * NH * T * 4
    ws = torch.empty(int(nws), dtype=torch.uint8, device=qkv.device)
    if doc_starts is not None:
        _chk_doc_starts(doc_starts, B, T)
        if not tile_scratch and int(lib.dg_attn_keep_bits_bytes(B, T, NH, H, dt_code(qkv.dtype))) > 0:
            raise ValueError("attn_bwd: doc_starts needs tile_scratch=True on a shape that takes the MFMA kernels")
    arg = None
    if fp8_out is not None:
        arg, q8, sinv = _attn_fp8_arg(fp8_out, tuple(qkv.shape), torch.float8_e5m2, qkv.device, only8=fp8_out_only)
    _attn_entry("dg_attn_bwd", (_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), _p(ws), ws.numel(), B, T, NH, H, float(scale), float(p),
                                _p(rng_state) if p > 0.0 else None, site, dt_code(qkv.dtype), _p(keep_bits),
                                keep_bits.numel() if keep_bits is not None else 0), arg, doc_starts)
    if arg is not None:
        dqkv.dg_fp8 = (q8, sinv)
        if fp8_out_only:
            dqkv.dg_unwritten = True
    return dqkv


def attn_decode(cache: Tensor, t: int, NH: int, H: int, scale: float) -> Tensor:
    """cache [B, Tcap, 3*NH*H]; returns the attention output of position t, [B, NH*H]."""
    _chk(cache, "cache")
    B, Tcap, W = cache.shape
    if W != 3 * NH * H:
        raise RuntimeError("attn_decode: cache width != 3*NH*H")
    out = torch.empty((B, NH * H), dtype=cache.dtype, device=cache.device)
    check(lib.dg_attn_decode(_p(cache), _p(out), B, Tcap, t, NH, H, float(scale), dt_code(cache.dtype), _stream()), "dg_attn_decode")
    return out


_NO_IGNORE = object()


def check_loss_options(label_smoothing=0.0, z_loss=0.0, ignore_index=_NO_IGNORE):
    """the checks of the loss options, plain Python, raised before anything touches a device: label_smoothing in [0, 1)
    (F.cross_entropy's label_smoothing), z_loss >= 0 and finite (the coefficient of logsumexp^2).  Returns both as floats.
    Called with ignore_index (F.cross_entropy's ignore_index: None, or an int that fits int64 -- never a bool or a float) it checks
    that too and returns all three."""
    if ignore_index is not _NO_IGNORE:
        if ignore_index is not None:
            if isinstance(ignore_index, bool) or not isinstance(ignore_index, numbers.Integral):
                raise ValueError(f"ignore_index must be None or an int, got {ignore_index!r}")
            ignore_index = int(ignore_index)
            if not -(1 << 63) <= ignore_index < (1 << 63):
                raise ValueError(f"ignore_index must fit int64, got {ignore_index!r}")
        return (*check_loss_options(label_smoothing, z_loss), ignore_index)
    out = []
    for name, x in (("label_smoothing", label_smoothing), ("z_loss", z_loss)):
        if isinstance(x, bool):
            raise ValueError(f"{name} must be a number, got {x!r}")
        try:
            out.append(float(x))
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be a number, got {x!r}") from None
    eps, zeta = out
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1), got {label_smoothing!r}")
    if not (math.isfinite(zeta) and zeta >= 0.0):
        raise ValueError(f"z_loss must be finite and >= 0, got {z_loss!r}")
    return eps, zeta


def _chk_inv_count(what: str, ignore_index, inv_count) -> None:
    if ignore_index is None:
        if inv_count is not None:
            raise ValueError(f"{what}: inv_count without ignore_index")
        return
    if inv_count is None:
        raise ValueError(f"{what}: ignore_index needs inv_count, the device's 1 / N (count_valid(targets, ignore_index)[1:])")
    _chk(inv_count, "inv_count", torch.float32)
    if inv_count.numel() < 1:
        raise ValueError(f"{what}: inv_count is empty")


def _ce_tensors(logits: Tensor, targets: Tensor, dlogits: Optional[Tensor], loss_rows: Optional[Tensor], logits_dtype=None, dlogits_dtype=None,
                need_dlogits: bool = True):
    """what the cross_entropy* functions share: the tensor checks and the loss_rows allocation.  Returns M, loss_rows and the
    leading dimension and dtype code of dlogits (0, DG_F32 without one)."""
    _chk(logits, "logits", logits_dtype, contiguous=False)  # fp32, or bf16 (large vocabularies: dlogits may then BE logits)
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError("cross_entropy: logits must be float32 or bfloat16")
    _chk(targets, "targets", torch.int64)
    M = logits.shape[0]
    if loss_rows is None:
        loss_rows = torch.empty((M,), dtype=torch.float32, device=logits.device)
    ldd, dcode = 0, DG_F32
    if dlogits is not None or need_dlogits:
        _chk(dlogits, "dlogits", dlogits_dtype, contiguous=False)
        ldd, dcode = _ld(dlogits), dt_code(dlogits.dtype)
    return M, loss_rows, ldd, dcode


def _ce_call(base: str, head: tuple, eps: float, zeta: Optional[float] = None, ignore_index: Optional[int] = None,
             inv_count: Optional[Tensor] = None) -> None:
    """base(*head), base_smooth(*head, eps[, zeta]) or base_ignore(*head, eps, zeta, ignore_index, inv_count), each with the stream last:
    the plain entry point when every option is zero.  zeta None: an entry point that has no z-loss."""
    opts = (eps,) if zeta is None else (eps, zeta)
    if ignore_index is not None:
        name, tail = base + "_ignore", (*opts, ignore_index, _p(inv_count))
    elif any(opts):
        name, tail = base + "_smooth", opts
    else:
        name, tail = base, ()
    check(getattr(lib, name)(*head, *tail, _stream()), name)


def cross_entropy(logits: Tensor, targets: Tensor, V: int, dlogits: Optional[Tensor] = None, grad_scale: float = 1.0,
                  grad_scale_dev: Optional[Tensor] = None, loss_rows: Optional[Tensor] = None, *,
                  label_smoothing: float = 0.0, z_loss: float = 0.0, ignore_index: Optional[int] = None,
                  inv_count: Optional[Tensor] = None) -> Tensor:
    """per-row objective (and, with dlogits, its gradient times grad_scale): the plain NLL, or with label_smoothing / z_loss
    lse - (1 - eps) x_t - (eps / V) sum x + z_loss lse^2 (dg_cross_entropy_smooth).  With ignore_index a row whose target equals it
    gets a zero objective and a zero gradient row, and the other gradient rows are also scaled by inv_count[0], the device's 1 / N
    (count_valid(targets, ignore_index)[1:]; dg_cross_entropy_ignore)."""
    eps, zeta, ignore_index = check_loss_options(label_smoothing, z_loss, ignore_index)
    _chk_inv_count("cross_entropy", ignore_index, inv_count)
    M, loss_rows, ldd, dcode = _ce_tensors(logits, targets, dlogits, loss_rows, need_dlogits=False)
    _ce_call("dg_cross_entropy", (_p(logits), dt_code(logits.dtype), _ld(logits), _p(targets), _p(loss_rows), _p(dlogits), ldd, dcode,
                                  float(grad_scale), _p(grad_scale_dev), M, V), eps, zeta, ignore_index, inv_count)
    return loss_rows


def cross_entropy_fp8(logits: Tensor, targets: Tensor, V: int, dlogits: Tensor, grad_scale: float, dlogits_fp8: Tensor, *,
                      label_smoothing: float = 0.0, ignore_index: Optional[int] = None) -> Tensor:
    """cross_entropy on bf16 logits (gradient in bf16, possibly in place) that also writes the gradient as e5m2 with the a-priori
    scale 57344 / grad_scale into dlogits_fp8 [M, ld8 >= V] (pad columns zeroed); dequantisation factor: grad_scale / 57344.
    label_smoothing keeps |dlogits| <= grad_scale, on which that scale rests; a z-loss does not, so there is no z_loss here; with
    ignore_index the bound would be the device's 1 / N, so that is refused too."""
    if ignore_index is not None:
        raise ValueError("cross_entropy_fp8 takes no ignore_index: its e5m2 gradient scale rests on |dlogits| <= grad_scale = 1 / M, and "
                         "with ignored rows the bound is 1 / N, which only the device knows")
    eps, _ = check_loss_options(label_smoothing, 0.0)
    M, loss_rows, ldd, _ = _ce_tensors(logits, targets, dlogits, None, torch.bfloat16, torch.bfloat16)
    _chk(dlogits_fp8, "dlogits_fp8", torch.float8_e5m2, contiguous=False)
    _ce_call("dg_cross_entropy_fp8", (_p(logits), _ld(logits), _p(targets), _p(loss_rows), _p(dlogits), ldd, float(grad_scale), M, V,
                                      _p(dlogits_fp8), _ld(dlogits_fp8)), eps)
    return loss_rows


def cross_entropy_fused_supported(logits: Tensor, dlogits: Tensor, n_partials: int) -> bool:
    return logits.dtype == torch.float32 and _ld(dlogits) <= 128 and 0 < n_partials <= 2048


def cross_entropy_fused(logits: Tensor, targets: Tensor, V: int, dlogits: Tensor, grad_scale: float, colsum_part: Optional[Tensor],
                        part_stride: int, n_partials: int, loss_scratch: Optional[Tensor], loss_out: Optional[Tensor], loss_scale: float,
                        loss_rows: Optional[Tensor] = None, *, label_smoothing: float = 0.0, z_loss: float = 0.0,
                        ignore_index: Optional[int] = None, inv_count: Optional[Tensor] = None) -> Tensor:
    """cross_entropy + column-sum partials of dlogits (n_partials rows of part_stride floats) + loss_out = loss_scale * sum(rows)
    in one launch (V <= 128).  loss_scratch: fp32 [n_partials + 1], its LAST word the arrival counter (zero before the first
    launch; the kernel leaves it at zero).  Returns the per-row losses (with label_smoothing / z_loss: the per-row objectives,
    and partials that no longer add up to zero once z_loss > 0).  With ignore_index: as in cross_entropy, the partials hold the
    rows that count and loss_out = loss_scale * inv_count[0] * sum(rows)."""
    eps, zeta, ignore_index = check_loss_options(label_smoothing, z_loss, ignore_index)
    _chk_inv_count("cross_entropy_fused", ignore_index, inv_count)
    M, loss_rows, ldd, dcode = _ce_tensors(logits, targets, dlogits, loss_rows, torch.float32)
    if colsum_part is not None:
        _chk(colsum_part, "colsum_part", torch.float32, contiguous=False)
    cnt = None
    if loss_out is not None:
        _chk(loss_out, "loss_out", torch.float32)
        _chk(loss_scratch, "loss_scratch", torch.float32)
        if loss_scratch.numel() < n_partials + 1:
            raise ValueError("cross_entropy_fused: loss_scratch needs n_partials + 1 words")
        cnt = loss_scratch.data_ptr() + 4 * n_partials
    _ce_call("dg_cross_entropy_fused", (_p(logits), _ld(logits), _p(targets), _p(loss_rows), _p(dlogits), ldd, dcode, float(grad_scale), M, V,
                                        _p(colsum_part), part_stride, n_partials, _p(loss_scratch) if loss_out is not None else None, cnt,
                                        _p(loss_out), float(loss_scale)), eps, zeta, ignore_index, inv_count)
    return loss_rows


def count_valid(targets: Tensor, ignore_index: int, out: Optional[Tensor] = None) -> Tensor:
    """fp32 [2] = {N, 1 / N}, N the number of targets that are not ignore_index (dg_ce_count_valid: one small launch, no sync)"""
    _, _, ignore_index = check_loss_options(ignore_index=ignore_index)
    if ignore_index is None:
        raise ValueError("count_valid: ignore_index must be an int")
    _chk(targets, "targets", torch.int64)
    if out is None:
        out = torch.empty((2,), dtype=torch.float32, device=targets.device)
    else:
        _chk(out, "out", torch.float32)
        if out.numel() < 2:
            raise ValueError("count_valid: out needs two words")
    check(lib.dg_ce_count_valid(_p(targets), targets.numel(), ignore_index, _p(out), _stream()), "dg_ce_count_valid")
    return out


def reduce_sum(x: Tensor, scale: float, out: Optional[Tensor] = None, scale_dev: Optional[Tensor] = None) -> Tensor:
    """out = scale * sum(x); with scale_dev (fp32, on the device) out = scale * scale_dev[0] * sum(x), the same order"""
    _chk(x, "x", torch.float32)
    if out is None:
        out = torch.empty((), dtype=torch.float32, device=x.device)
    if scale_dev is not None:
        _chk(scale_dev, "scale_dev", torch.float32)
        check(lib.dg_reduce_sum_scaled(_p(x), x.numel(), float(scale), _p(scale_dev), _p(out), _stream()), "dg_reduce_sum_scaled")
        return out
    check(lib.dg_reduce_sum(_p(x), x.numel(), float(scale), _p(out), _stream()), "dg_reduce_sum")
    return out


def softmax_rows(logits: Tensor) -> Tensor:
    _chk(logits, "logits", torch.float32, contiguous=False)
    M, V = logits.shape
    probs = torch.empty((M, V), dtype=torch.float32, device=logits.device)
    check(lib.dg_softmax_rows(_p(logits), _ld(logits), _p(probs), V, M, V, _stream()), "dg_softmax_rows")
    return probs


def _f32_bits(x: float) -> int:
    import struct
    return struct.unpack("<i", struct.pack("<f", x))[0]


def new_sample_params(temperature: float, top_k: Optional[int], device, *, top_p: Optional[float] = None,
                      min_p: Optional[float] = None, four: bool = False) -> Tensor:
    """device {float inv_temp, int32 top_k} of sample_rows (stored as two int32 bit patterns).  temperature 0 = greedy
    (inv_temp 0); top_k None / 0 = off.  inv_temp is 1 / temperature rounded to fp32.
    With a top_p or a min_p, or with four=True (what dg_sample_rows_control and a captured sampler take): the four-word block
    {inv_temp, top_k, float top_p, float min_p} of dg_sample_rows_nucleus (top_p None = 1 = off, min_p None = 0 = off: the one
    place where that is filled in)."""
    inv = 0.0 if temperature == 0 else 1.0 / float(temperature)
    words = [_f32_bits(inv), int(top_k or 0)]
    if four or top_p is not None or min_p is not None:
        # a top_p below the smallest fp32 must not round to 0, which the kernel takes as "off": it keeps the maximum alone
        words += [_f32_bits(1.0 if top_p is None else max(float(top_p), 2.0 ** -149)), _f32_bits(0.0 if min_p is None else float(min_p))]
    return torch.tensor(words, dtype=torch.int32, device=device)


SAMPLE_MAX_STOP = 8          # DG_SAMPLE_MAX_STOP
SAMPLE_CONTROL_WORDS = 16


def new_sample_control(*, repetition_penalty: float = 1.0, presence_penalty: float = 0.0, frequency_penalty: float = 0.0,
                       stop_tokens=(), pad_token: Optional[int] = None, use_bias: bool = False, device=None) -> Tensor:
    """the 16-word control block of dg_sample_rows_control as int32 bit patterns: {float inv_rep, float rep, float presence,
    float frequency, int32 use_bias, int32 n_stop, int32 pad_id, 0, int32 stop[8]}.  inv_rep is 1 / rep rounded to fp32 once,
    here; pad_token None = the first stop token (0 without one); unused stop slots hold -1."""
    stop = [int(t) for t in stop_tokens]
    if len(stop) > SAMPLE_MAX_STOP:
        raise ValueError(f"new_sample_control: at most {SAMPLE_MAX_STOP} stop tokens, got {len(stop)}")
    rep = float(repetition_penalty)
    pad = int(pad_token) if pad_token is not None else (stop[0] if stop else 0)
    words = [_f32_bits(1.0 / rep), _f32_bits(rep), _f32_bits(float(presence_penalty)), _f32_bits(float(frequency_penalty)),
             int(bool(use_bias)), len(stop), pad, 0] + stop + [-1] * (SAMPLE_MAX_STOP - len(stop))
    return torch.tensor(words, dtype=torch.int32, device=device)


def _chk_counts(what: str, counts: Tensor, M: int, V: int) -> None:
    _chk(counts, "counts", torch.int32, contiguous=False)
    if counts.dim() != 2 or counts.shape[0] != M or counts.shape[1] < V or counts.stride(1) != 1:
        raise RuntimeError(f"{what}: counts must be int32 [M = {M}, >= V = {V}]")


def token_counts(ids: Tensor, n, V: int, counts: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    """int32 [M, V] (or the given counts [M, >= V]): how often each token occurs in ids[m, :n] (dg_token_counts; ids int64 [M, cap],
    rows may be strided, clamped to [0, V) as the embedding does).  accumulate=False zeroes the counts first.
    n may also be a device int32 tensor [M] of any stride, a prefix length per row, clamped to [0, cap] (dg_token_counts_rows)."""
    _chk(ids, "ids", torch.int64, contiguous=False)
    per_row = isinstance(n, torch.Tensor)
    if ids.dim() != 2 or ids.stride(1) != 1 or not (per_row or 0 <= n <= ids.shape[1]):
        raise RuntimeError("token_counts: ids must be [M, capacity >= n] with unit column stride")
    M = ids.shape[0]
    if per_row:
        _chk(n, "n", torch.int32, contiguous=False)
        # the kernel clamps a row's n to the row stride: whole rows only, so that the clamp is the capacity
        if n.dim() != 1 or n.shape[0] != M or n.stride(0) < 0 or _ld(ids) != ids.shape[1]:
            raise RuntimeError(f"token_counts: a per-row n must be int32 [M = {M}] and ids whole rows [M, capacity]")
    if counts is None:
        if accumulate:
            raise ValueError("token_counts: accumulate=True needs counts")
        counts = torch.empty((M, V), dtype=torch.int32, device=ids.device)
    _chk_counts("token_counts", counts, M, V)
    if per_row:
        check(lib.dg_token_counts_rows(_p(ids), ids.shape[1], M, _p(n), n.stride(0), int(V), _p(counts), _ld(counts),
                                       int(bool(accumulate)), _stream()), "dg_token_counts_rows")
        return counts
    check(lib.dg_token_counts(_p(ids), max(_ld(ids), n), M, int(n), int(V), _p(counts), _ld(counts), int(bool(accumulate)), _stream()),
          "dg_token_counts")
    return counts


def sample_rows(logits: Tensor, state: Optional[Tensor] = None, params: Optional[Tensor] = None, *, seed: Optional[int] = None,
                L: Optional[int] = None, temperature: float = 1.0, top_k: Optional[int] = None, ids: Optional[Tensor] = None,
                tokens: bool = True, probs: bool = False, top_p: Optional[float] = None, min_p: Optional[float] = None,
                control: Optional[Tensor] = None, bias: Optional[Tensor] = None, counts: Optional[Tensor] = None,
                lengths: Optional[Tensor] = None, spans: Optional[Tensor] = None):
    """one token per row of fp32 logits [M, V] (dg_sample_rows, or dg_sample_rows_nucleus when params has four words;
    include/drakegpt_hip.h states the semantics).
    control: new_sample_control(...) -- dg_sample_rows_control: penalties on counts int32 [M, >= V] (the kernel adds the token
    it writes), bias fp32 [V] (read when the block's use_bias is set), lengths int32 [M] (stop tokens; needs ids).  The
    parameter block built here then always has four words.  Without control: bias / counts / lengths are refused.
    spans: int32 [M, 2] {first, end} per row -- dg_sample_rows_ragged: a row with L < first keeps the prompt token that ids[m, L]
    holds and is left alone, a row that writes position end - 1 is finished.  Needs control, lengths and the 2-D ids.
    state: decode state int32[4] {seed_lo, seed_hi, L, 0} (new_rng_state(seed, device, step=L)); built from seed / L when None.
    params: new_sample_params(...); built from temperature / top_k / top_p / min_p when None.
    ids [B, cap] int64: row m's token is written to ids[m, L] by the kernel (nothing is returned for it); otherwise, with
    tokens=True, a new int64 [M] tensor is returned.  probs=True also returns the filtered distribution [M, V].
    Returns tokens, probs, (tokens, probs) or None according to what was asked for."""
    _chk(logits, "logits", torch.float32, contiguous=False)
    if logits.dim() != 2:
        raise RuntimeError("sample_rows: logits must be [M, V]")
    M, V = logits.shape
    want_tok = tokens or ids is not None
    if not want_tok and not probs:
        raise ValueError("sample_rows: nothing to compute (tokens=False, probs=False)")
    if control is None and (bias is not None or counts is not None or lengths is not None):
        raise ValueError("sample_rows: bias / counts / lengths need control=new_sample_control(...)")
    if spans is not None and (control is None or lengths is None or ids is None):
        raise ValueError("sample_rows: spans need control=, lengths= and ids=")
    if params is None:
        params = new_sample_params(temperature, top_k, logits.device, top_p=top_p, min_p=min_p, four=control is not None)
    _chk(params, "params", torch.int32)
    if control is not None:
        _chk(control, "control", torch.int32)
        if control.numel() != SAMPLE_CONTROL_WORDS or params.numel() != 4:
            raise RuntimeError("sample_rows: control must hold 16 words and comes with the four-word params")
        if bias is not None:
            _chk(bias, "bias", torch.float32)
            if bias.numel() != V:
                raise RuntimeError(f"sample_rows: bias must be fp32 [V = {V}]")
        if counts is not None:
            _chk_counts("sample_rows", counts, M, V)
        if lengths is not None:
            _chk(lengths, "lengths", torch.int32)
            if lengths.numel() != M or ids is None:
                raise RuntimeError(f"sample_rows: lengths must be int32 [M = {M}] and needs ids=")
        if spans is not None:
            _chk(spans, "spans", torch.int32)
            if tuple(spans.shape) != (M, 2):
                raise RuntimeError(f"sample_rows: spans must be int32 [M = {M}, 2]")
    if params.numel() not in (2, 4):
        raise RuntimeError("sample_rows: params must hold {inv_temp, top_k} or {inv_temp, top_k, top_p, min_p}")
    # the one place that picks the entry, from (spans given, control given, block length); control takes its operands after the rest
    name = ("dg_sample_rows_ragged" if spans is not None else "dg_sample_rows_control" if control is not None
            else "dg_sample_rows" if params.numel() == 2 else "dg_sample_rows_nucleus")
    if want_tok:
        if state is None:
            if seed is None or L is None:
                raise ValueError("sample_rows: tokens need a decode state, or seed= and L=")
            state = new_rng_state(int(seed), logits.device, step=int(L))
        _chk(state, "state", torch.int32)
        if state.numel() != 4:
            raise RuntimeError("sample_rows: state must be int32[4]")
    out_tok, ld_ids, tok_ptr = None, 0, None
    if ids is not None:
        _chk(ids, "ids", torch.int64)
        if ids.dim() != 2 or ids.shape[0] != M:
            raise RuntimeError(f"sample_rows: ids must be [M = {M}, capacity]")
        ld_ids, tok_ptr = ids.shape[1], _p(ids)
    elif tokens:
        out_tok = torch.empty((M,), dtype=torch.int64, device=logits.device)
        tok_ptr = _p(out_tok)
    p_out = torch.empty((M, V), dtype=torch.float32, device=logits.device) if probs else None
    extra = () if control is None else (_p(control), _p(bias), _p(counts), 0 if counts is None else _ld(counts), _p(lengths))
    if spans is not None:
        extra += (_p(spans),)
    check(getattr(lib, name)(_p(logits), _ld(logits), M, V, _p(state) if want_tok else None, _p(params), tok_ptr, ld_ids, _p(p_out), V,
                             *extra, _stream()), name)
    if out_tok is not None and probs:
        return out_tok, p_out
    return out_tok if out_tok is not None else p_out


LOGPROBS_MAX_TOP = 20        # DG_LOGPROBS_MAX_TOP


def check_top_logprobs(top_n, what: str = "top_n") -> int:
    """an integer in [0, LOGPROBS_MAX_TOP]: plain Python, raised before anything touches a device"""
    if isinstance(top_n, bool) or not isinstance(top_n, numbers.Integral) or not 0 <= int(top_n) <= LOGPROBS_MAX_TOP:
        raise ValueError(f"{what} must be an integer in [0, {LOGPROBS_MAX_TOP}], got {top_n!r}")
    return int(top_n)


def token_logprobs(logits: Tensor, tokens: Tensor, *, top_n=0, rank: bool = False, state: Optional[Tensor] = None,
                   lengths: Optional[Tensor] = None, spans: Optional[Tensor] = None, out: Optional[Tensor] = None,
                   out_rank: Optional[Tensor] = None, out_top_ids: Optional[Tensor] = None, out_top_lp: Optional[Tensor] = None):
    """log_softmax of the raw logits [M, V] (fp32 or bf16) at one token per row (dg_token_logprobs; include/drakegpt_hip.h states
    the arithmetic and its order).  tokens int64 [M]: returns lp fp32 [M]; with rank=True also the token's rank int32 [M] (0 = the
    greedy pick); with top_n > 0 also the top_n most likely ids int32 [M, top_n] and their lp fp32 [M, top_n] (-1 / -inf where the
    row has fewer finite entries).  Returns lp alone, or a tuple (lp, [rank,] [top_ids, top_lp]) in that order.
    The decode form, for a step that a graph replays: tokens int64 [M, cap] with state (the decode state, L = state[2]): the token
    is tokens[m, L], every output is one the caller owns -- out fp32 [M, cap], out_rank int32 [M, cap], out_top_ids int32 /
    out_top_lp fp32 [M, cap, LOGPROBS_MAX_TOP], each optional -- written at column L, top_n is a device int32 word that the kernel
    reads, and rows that lengths [M] / spans [M, 2] (the sampler's) mark as finished before L or as forced are left untouched.
    Nothing is returned."""
    _chk(logits, "logits", contiguous=False)
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"token_logprobs: logits must be float32 or bfloat16, got {logits.dtype}")
    if logits.dim() != 2:
        raise RuntimeError("token_logprobs: logits must be [M, V]")
    M, V = logits.shape
    _chk(tokens, "tokens", torch.int64)
    dev = logits.device
    if tokens.dim() == 2:
        if state is None or tokens.shape[0] != M or tokens.shape[1] < 1:
            raise RuntimeError(f"token_logprobs: tokens [M = {M}, cap] come with the decode state")
        _chk(state, "state", torch.int32)
        if state.numel() != 4:
            raise RuntimeError("token_logprobs: state must be int32[4]")
        cap = tokens.shape[1]
        for t, name, dt, shape in ((out, "out", torch.float32, (M, cap)), (out_rank, "out_rank", torch.int32, (M, cap)),
                                   (out_top_ids, "out_top_ids", torch.int32, (M, cap, LOGPROBS_MAX_TOP)),
                                   (out_top_lp, "out_top_lp", torch.float32, (M, cap, LOGPROBS_MAX_TOP)),
                                   (lengths, "lengths", torch.int32, (M,)), (spans, "spans", torch.int32, (M, 2))):
            if t is not None:
                _chk(t, name, dt)
                if tuple(t.shape) != shape:
                    raise RuntimeError(f"token_logprobs: {name} must be {shape}, got {tuple(t.shape)}")
        if (out_top_ids is None) != (out_top_lp is None):
            raise ValueError("token_logprobs: out_top_ids and out_top_lp come together")
        if out_top_ids is not None:
            if not isinstance(top_n, torch.Tensor):
                raise ValueError("token_logprobs: the decode form reads top_n from a device int32 word")
            _chk(top_n, "top_n", torch.int32)
        check(lib.dg_token_logprobs(_p(logits), dt_code(logits.dtype), _ld(logits), M, V, _p(tokens), cap, _p(state), _p(lengths),
                                    _p(spans), _p(top_n) if out_top_ids is not None else None, _p(out), _p(out_rank),
                                    _p(out_top_ids), _p(out_top_lp), _stream()), "dg_token_logprobs")
        return None
    if tokens.dim() != 1 or tokens.shape[0] != M:
        raise RuntimeError(f"token_logprobs: tokens must be int64 [M = {M}]")
    if state is not None or lengths is not None or spans is not None or any(
            t is not None for t in (out, out_rank, out_top_ids, out_top_lp)):
        raise ValueError("token_logprobs: state, lengths, spans and the out tensors belong to the decode form (tokens [M, cap])")
    n = check_top_logprobs(top_n, "token_logprobs: top_n")
    lp = torch.empty(M, dtype=torch.float32, device=dev)
    rk = torch.empty(M, dtype=torch.int32, device=dev) if rank else None
    ti = torch.empty((M, LOGPROBS_MAX_TOP), dtype=torch.int32, device=dev) if n else None
    tl = torch.empty((M, LOGPROBS_MAX_TOP), dtype=torch.float32, device=dev) if n else None
    n_dev = torch.tensor([n], dtype=torch.int32, device=dev) if n else None
    check(lib.dg_token_logprobs(_p(logits), dt_code(logits.dtype), _ld(logits), M, V, _p(tokens), 0, None, None, None, _p(n_dev),
                                _p(lp), _p(rk), _p(ti), _p(tl), _stream()), "dg_token_logprobs")
    res = (lp,) + ((rk,) if rank else ()) + ((ti[:, :n], tl[:, :n]) if n else ())
    return lp if len(res) == 1 else res


def embed_window(ids: Tensor, state: Tensor, tok: Tensor, pos: Tensor, mode: int, out: Optional[Tensor] = None) -> Tensor:
    """the embedding of a decode step with the position L = state[2] read on the device (dg_embed_window).
    mode 0: [B, C] = tok[ids[:, L-1]] + pos[L-1];  mode 1: [B, Tw, C] = tok[ids[:, L-Tw:L]] + pos, Tw = rows of pos."""
    _chk(ids, "ids", torch.int64)
    _chk(state, "state", torch.int32)
    _chk(tok, "tok", torch.float32)
    _chk(pos, "pos", torch.float32)
    if ids.dim() != 2 or state.numel() != 4 or mode not in (0, 1):
        raise RuntimeError("embed_window: ids must be [B, capacity], state int32[4], mode 0 or 1")
    B, cap = ids.shape
    V, Cd = tok.shape
    Tw = pos.shape[0]
    if pos.shape[1] != Cd:
        raise RuntimeError("embed_window: tok and pos widths differ")
    shape = (B, Cd) if mode == 0 else (B, Tw, Cd)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=ids.device)
    else:
        _chk(out, "out", torch.float32)
        if tuple(out.shape) != shape:
            raise RuntimeError(f"embed_window: out must be {shape}")
    check(lib.dg_embed_window(_p(ids), cap, _p(state), _p(tok), _p(pos), _p(out), B, Tw, Cd, V, mode, _stream()), "dg_embed_window")
    return out


def attn_decode_append(row: Tensor, cache: Tensor, state: Tensor, NH: int, H: int, scale: float,
                       out: Optional[Tensor] = None) -> Tensor:
    """attn_decode at position t = state[2] - 1 read on the device: row [B, 3*NH*H] (the new token's q/k/v) is written into
    cache[:, t] and attended over keys 0..t; returns [B, NH*H].  t >= Tcap: nothing happens (out keeps its contents)."""
    _chk(cache, "cache")
    _chk(row, "row", cache.dtype)
    _chk(state, "state", torch.int32)
    B, Tcap, W = cache.shape
    if W != 3 * NH * H or tuple(row.shape) != (B, W) or state.numel() != 4:
        raise RuntimeError("attn_decode_append: cache must be [B, Tcap, 3*NH*H], row [B, 3*NH*H], state int32[4]")
    if out is None:
        out = torch.empty((B, NH * H), dtype=cache.dtype, device=cache.device)
    else:
        _chk(out, "out", cache.dtype)
        if tuple(out.shape) != (B, NH * H):
            raise RuntimeError("attn_decode_append: out must be [B, NH*H]")
    check(lib.dg_attn_decode_append(_p(row), _p(cache), _p(out), _p(state), B, Tcap, NH, H, float(scale), dt_code(cache.dtype),
                                    _stream()), "dg_attn_decode_append")
    return out


def adamw_step(p: Tensor, g: Tensor, m: Tensor, v: Tensor, hyper: Tensor, rng_state: Tensor, grad_scale: float = 1.0,
               shadow_bf16: Optional[Tensor] = None, n: Optional[int] = None, advance: bool = False, *,
               clip: Optional[Tensor] = None, lr_table: Optional[Tensor] = None, no_decay_bits: Optional[Tensor] = None,
               ema: Optional[Tensor] = None, ema_hyper: Optional[Tensor] = None, guard: Optional[Tensor] = None,
               data_state: Optional[Tensor] = None) -> None:
    """One fused AdamW launch over the first n elements (default: all) of the flat buffers.  The entry is the first of
    dg_adamw_step_guard / _ema / _sched / _clip / dg_adamw_step that takes everything given; an operand that is None costs nothing.
    advance: the launch also moves the step word of rng_state on (what state_advance does, without its launch).
    clip: a device fp32 scalar, the clipping coefficient written by grad_norm (out[1:2]); the step then applies g * grad_scale * coef
    and g itself stays unclipped.
    lr_table: a device fp32 vector; the update uses lr_table[min(step word, len - 1)] instead of hyper[0].
    no_decay_bits: the bitmap of new_no_decay_bits(ranges, n, device); elements of a set granule see weight_decay = 0.
    ema (with ema_hyper = new_ema_hyper(decay, warmup, device)): the launch also moves this moving average of the weights on
    (ema += (p_new - ema) * (1 - d_s) by the step word it reads; step word 0: ema = p_new); p, m, v, the shadow and the state words
    are the ones the launch without it writes.
    guard: the update guard grad_norm(guard=...) has just written (new_update_guard).  guard[0] == 1: the bits of the launch without
    it.  guard[0] == 0: the update is skipped -- no buffer is read or written and rng_state's step word stays.  data_state (with
    guard and advance): a second 4-word state whose step word the launch moves on in either case (the data side of a training
    step: dropout key, staged offset row, fp8 amax slot)."""
    # the checks, every one for every entry: what the library indexes and cannot check itself
    for t, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v"), (hyper, "hyper")):
        _chk(t, nm, torch.float32)
    n = p.numel() if n is None else n
    if ema is None and ema_hyper is not None:
        raise ValueError("adamw_step: ema_hyper goes with ema")
    if guard is None and data_state is not None:
        raise ValueError("adamw_step: data_state goes with guard")
    if ema is not None and ema_hyper is None:
        raise ValueError("adamw_step: ema needs ema_hyper (new_ema_hyper)")
    streams = {"p": p, "g": g, "m": m, "v": v}
    _chk(rng_state, "rng_state", torch.int32)
    for t, nm, dtype in ((guard, "guard", torch.int32), (ema, "ema", torch.float32), (ema_hyper, "ema_hyper", torch.float32),
                         (lr_table, "lr_table", torch.float32), (no_decay_bits, "no_decay_bits", torch.int32), (clip, "clip", torch.float32),
                         (data_state, "data_state", torch.int32)):
        if t is not None:
            _chk(t, nm, dtype)
    if rng_state.numel() < 4 or (guard is not None and guard.numel() < 4):
        raise ValueError("adamw_step: guard and rng_state need 4 words each (new_update_guard, new_rng_state)")
    if ema is not None:
        if ema_hyper.numel() < 2:
            raise ValueError("adamw_step: ema_hyper needs 2 floats {decay, warmup} (new_ema_hyper)")
        streams["ema"] = ema
    if n < 1 or any(n > t.numel() for t in streams.values()):
        raise ValueError(f"adamw_step: n = {n} does not fit {', '.join(streams)}")
    if lr_table is not None and (lr_table.dim() != 1 or lr_table.numel() < 1):
        raise ValueError("adamw_step: lr_table must be a 1-D tensor with at least one entry")
    if no_decay_bits is not None and no_decay_bits.numel() < no_decay_words(n):
        raise ValueError(f"adamw_step: no_decay_bits needs {no_decay_words(n)} words for n = {n}, got {no_decay_bits.numel()}")
    if shadow_bf16 is not None and shadow_bf16.numel() < n:
        raise ValueError(f"adamw_step: shadow_bf16 holds {shadow_bf16.numel()} elements, n = {n}")
    if data_state is not None and (data_state.numel() < 4 or data_state.data_ptr() == rng_state.data_ptr()):
        raise ValueError("adamw_step: data_state needs 4 words of its own (not rng_state)")
    # the route: the first entry that takes everything given; each entry's arguments are the shared prefix, its own tail, the stream
    sched = (_p(clip), _p(lr_table), 0 if lr_table is None else lr_table.numel(), _p(no_decay_bits), _p(shadow_bf16), int(advance))
    if guard is not None:
        entry, tail = "dg_adamw_step_guard", sched + (_p(ema), _p(ema_hyper), _p(guard), _p(data_state))
    elif ema is not None:
        entry, tail = "dg_adamw_step_ema", sched + (_p(ema), _p(ema_hyper))
    elif lr_table is not None or no_decay_bits is not None:
        entry, tail = "dg_adamw_step_sched", sched
    elif clip is not None:
        entry, tail = "dg_adamw_step_clip", (_p(clip), _p(shadow_bf16), int(advance))
    else:
        entry, tail = "dg_adamw_step", (_p(shadow_bf16), int(advance))
    check(getattr(lib, entry)(_p(p), _p(g), _p(m), _p(v), n, _p(hyper), _p(rng_state), float(grad_scale), *tail, _stream()), entry)


def check_ema_options(decay=None, warmup=False):
    """the checks of the two EMA options, plain Python, raised before anything touches a device: decay None (no moving average) or
    a number with 0 < decay < 1 (no bools, no NaN); warmup (d_s = min(decay, (s + 1) / (s + 10))) goes with a decay.  Returns the
    decay as None or a float."""
    if decay is None:
        if warmup:
            raise ValueError("ema_warmup goes with ema_decay")
        return None
    if isinstance(decay, bool):
        raise ValueError(f"ema_decay must be a number in (0, 1), got {decay!r}")
    try:
        d = float(decay)
    except (TypeError, ValueError):
        raise ValueError(f"ema_decay must be a number in (0, 1), got {decay!r}") from None
    if not 0.0 < d < 1.0:          # (NaN fails both comparisons)
        raise ValueError(f"ema_decay must be a number in (0, 1), got {decay!r}")
    if float(torch.tensor(d, dtype=torch.float32)) >= 1.0:
        raise ValueError(f"ema_decay {decay!r} rounds to 1 in fp32: the average would never move")
    return d


def new_ema_hyper(decay, warmup, device) -> Tensor:
    """device fp32 {decay, warmup != 0} for adamw_step(ema=...): read by the launch, so writing it changes the decay of a captured graph"""
    d = check_ema_options(decay, warmup)
    if d is None:
        raise ValueError("new_ema_hyper: ema_decay is None")
    return torch.tensor([d, 1.0 if warmup else 0.0], dtype=torch.float32, device=device)


def swap_(a: Tensor, b: Tensor, n: Optional[int] = None) -> None:
    """exchange the first n elements (default: all) of two fp32 buffers in one launch (dg_swap_f32)"""
    _chk(a, "a", torch.float32)
    _chk(b, "b", torch.float32)
    n = min(a.numel(), b.numel()) if n is None else int(n)
    if n < 1 or n > a.numel() or n > b.numel():
        raise ValueError(f"swap_: n = {n} does not fit a ({a.numel()}) and b ({b.numel()})")
    lo, hi = sorted((a.data_ptr(), b.data_ptr()))
    if lo + 4 * n > hi:
        raise ValueError("swap_: a and b overlap")
    check(lib.dg_swap_f32(_p(a), _p(b), n, _stream()), "dg_swap_f32")


NO_DECAY_GRANULE = 64   # floats per bit of the no-decay bitmap: ALIGN of engine.py and _ALIGN of optim.py


def no_decay_words(n: int) -> int:
    """uint32 words of the no-decay bitmap over n floats: ceil(ceil(n / 64) / 32)"""
    return ((n + NO_DECAY_GRANULE - 1) // NO_DECAY_GRANULE + 31) // 32


def new_no_decay_bits(ranges, n: int, device) -> Tensor:
    """the bitmap dg_adamw_step_sched reads (uint32 words stored as int32 bit patterns): bit (G & 31) of word (G >> 5) is set
    when the granule of elements [64 G, 64 G + 64) lies in one of the [lo, hi) element ranges.  A range has to start on a granule
    and end on one or at n: half a granule cannot be kept out of weight decay."""
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"new_no_decay_bits: n must be an integer >= 1, got {n!r}")
    words = [0] * no_decay_words(n)
    for lo, hi in ranges:
        lo, hi = int(lo), int(hi)
        if not 0 <= lo <= hi <= n:
            raise ValueError(f"new_no_decay_bits: range [{lo}, {hi}) does not lie in [0, {n})")
        if lo % NO_DECAY_GRANULE or (hi % NO_DECAY_GRANULE and hi != n):
            raise ValueError(f"new_no_decay_bits: range [{lo}, {hi}) must start on a multiple of {NO_DECAY_GRANULE} and end on one or at n = {n}")
        for G in range(lo // NO_DECAY_GRANULE, (hi + NO_DECAY_GRANULE - 1) // NO_DECAY_GRANULE):
            words[G >> 5] |= 1 << (G & 31)
    words = [w - (1 << 32) if w >= (1 << 31) else w for w in words]
    return torch.tensor(words, dtype=torch.int32, device=device)


def grad_norm_workspace(gs, device) -> Tensor:
    """the fp64 partial sums grad_norm needs for the flat gradients gs (one range per buffer); reusable across steps"""
    return torch.empty(sum(int(lib.dg_sumsq_parts(g.numel())) for g in gs), dtype=torch.float64, device=device)


GUARD_NONFINITE_LIMIT = float(torch.finfo(torch.float32).max)   # the limit that guards non-finite gradients alone (+inf would pass an Inf norm)


def check_guard_options(skip_nonfinite=False, skip_grad_norm=None):
    """the checks of the two update-guard options, plain Python, raised before anything touches a device: skip_nonfinite a bool;
    skip_grad_norm None or a finite number > 0 (no bools, no NaN), the largest global gradient norm whose update is applied.
    skip_grad_norm implies skip_nonfinite (a non-finite norm fails the comparison too).  Returns (on, limit): whether the guard
    is on, and the fp32 limit to stage (None when off; FLT_MAX with skip_nonfinite alone)."""
    if not isinstance(skip_nonfinite, bool):
        raise ValueError(f"skip_nonfinite must be a bool, got {skip_nonfinite!r}")
    if skip_grad_norm is None:
        return skip_nonfinite, (GUARD_NONFINITE_LIMIT if skip_nonfinite else None)
    if isinstance(skip_grad_norm, bool):
        raise ValueError(f"skip_grad_norm must be a finite number > 0 or None, got {skip_grad_norm!r}")
    try:
        f = float(skip_grad_norm)
    except (TypeError, ValueError):
        raise ValueError(f"skip_grad_norm must be a finite number > 0 or None, got {skip_grad_norm!r}") from None
    if not (0.0 < f < math.inf):          # (NaN fails both comparisons)
        raise ValueError(f"skip_grad_norm must be a finite number > 0 or None, got {skip_grad_norm!r}")
    return True, min(f, GUARD_NONFINITE_LIMIT)


def new_update_guard(device) -> Tensor:
    """device uint32[4] = {apply = 1, total skipped = 0, consecutive skipped = 0, spare} for grad_norm(guard=...) and
    adamw_step(guard=...) (stored as int32)"""
    return torch.tensor([1, 0, 0, 0], dtype=torch.int32, device=device)


def grad_norm(gs, grad_scale: float, max_norm: Optional[Tensor], out: Tensor, work: Optional[Tensor] = None, *,
              guard: Optional[Tensor] = None, limit: Optional[Tensor] = None, loss: Optional[Tensor] = None) -> Tensor:
    """global 2-norm of the flat fp32 gradients gs (a tensor or a list of them: one norm over all) times grad_scale, and the
    clipping coefficient -- the norm and coef of torch.nn.utils.clip_grad_norm_(params, max_norm) (norm_type 2), without touching
    the gradients.  Writes out[0] = total_norm, out[1] = min(1, max_norm / (total_norm + 1e-6)); max_norm is a device fp32 scalar.
    One dg_sumsq_partials launch per buffer and one dg_grad_norm_finalize launch; the result is bitwise reproducible.
    guard (new_update_guard) with limit (a device fp32 scalar) and optionally loss (a device fp32 scalar): the finalize launch is
    dg_grad_norm_finalize_guard -- the same out bits, and guard = {apply, total skipped, consecutive skipped}: apply = total_norm
    <= limit and loss is finite.  max_norm may then be None (no clipping: out[1] is not written).  The sum of squares is taken in
    fp32, so an element beyond 1.8e19 in magnitude reads as non-finite (as in all_finite).  Without guard: the calls as they were."""
    gs = [gs] if isinstance(gs, Tensor) else list(gs)
    for i, g in enumerate(gs):
        _chk(g, f"gs[{i}]", torch.float32)
    if guard is None:
        if limit is not None or loss is not None:
            raise ValueError("grad_norm: limit and loss go with guard")
        _chk(max_norm, "max_norm", torch.float32)
    else:
        if limit is None:
            raise ValueError("grad_norm: guard needs limit (a device fp32 scalar)")
        _chk(guard, "guard", torch.int32)
        if guard.numel() < 4:
            raise ValueError("grad_norm: guard needs 4 words {apply, skipped, consecutive, spare} (new_update_guard)")
        for t, nm in ((max_norm, "max_norm"), (limit, "limit"), (loss, "loss")):
            if t is not None:
                _chk(t, nm, torch.float32)
                if t.numel() < 1:
                    raise ValueError(f"grad_norm: {nm} needs 1 float")
    _chk(out, "out", torch.float32)
    if out.numel() < 2:
        raise ValueError("grad_norm: out needs 2 floats {total_norm, coef}")
    if work is None:
        work = grad_norm_workspace(gs, out.device)
    parts = [int(lib.dg_sumsq_parts(g.numel())) for g in gs]
    if work.dtype != torch.float64 or work.numel() < sum(parts):
        raise ValueError(f"grad_norm: work must be float64 with at least {sum(parts)} elements")
    base = 0
    for g, k in zip(gs, parts):
        check(lib.dg_sumsq_partials(_p(g), g.numel(), work.data_ptr() + 8 * base, _stream()), "dg_sumsq_partials")
        base += k
    if guard is None:
        check(lib.dg_grad_norm_finalize(_p(work), base, float(grad_scale), _p(max_norm), _p(out), _stream()), "dg_grad_norm_finalize")
    else:
        check(lib.dg_grad_norm_finalize_guard(_p(work), base, float(grad_scale), _p(max_norm), _p(out), _p(limit), _p(loss), _p(guard),
                                              _stream()), "dg_grad_norm_finalize_guard")
    return out


def all_finite(ts, work: Optional[Tensor] = None) -> bool:
    """True when every element of the fp32 device tensors ts is finite: the fp64 partial sums of squares dg_sumsq_partials
    leaves (grad_norm's first pass) are finite when every fp32 element under them is.  (The kernel squares in fp32, so a finite
    element beyond 1.8e19 in magnitude also reads as not finite: as a weight or an Adam moment that is a diverged run too.)
    One launch per tensor (16-byte aligned, as every flat buffer is), one device round trip; not for the hot path."""
    ts = [ts] if isinstance(ts, Tensor) else list(ts)
    for i, t in enumerate(ts):
        _chk(t, f"ts[{i}]", torch.float32)
    ts = [t for t in ts if t.numel()]
    if not ts:
        return True
    need = sum(int(lib.dg_sumsq_parts(t.numel())) for t in ts)
    if work is None or work.dtype != torch.float64 or work.numel() < need:
        work = torch.empty(need, dtype=torch.float64, device=ts[0].device)
    base = 0
    for t in ts:
        check(lib.dg_sumsq_partials(_p(t), t.numel(), work.data_ptr() + 8 * base, _stream()), "dg_sumsq_partials")
        base += int(lib.dg_sumsq_parts(t.numel()))
    return bool(torch.isfinite(work[:base]).all().item())


def new_accum_ctl(k: int, device) -> Tensor:
    """device uint32[4] = {j = 0, k, arrival counter = 0, 0} for grad_accumulate (stored as int32); k = accum_steps is validated here,
    on the host: the launch itself never looks at it again"""
    if isinstance(k, bool) or not isinstance(k, int) or k < 1 or k >= (1 << 31):
        raise ValueError(f"new_accum_ctl: k must be an integer >= 1, got {k!r}")
    return torch.tensor([0, k, 0, 0], dtype=torch.int32, device=device)


def grad_accumulate(acc: Tensor, g: Tensor, n: Optional[int], ctl: Tensor, loss: Optional[Tensor] = None,
                    loss_out: Optional[Tensor] = None, rng_state: Optional[Tensor] = None) -> None:
    """one micro-step of gradient accumulation (dg_grad_accumulate): acc[0, n) = g (ctl[0] == 0) or acc + g (one fp32 add per
    element), loss_out = {running sum of loss, its mean over k on the last micro-step}; the launch moves ctl[0] on to
    (j + 1) mod k and, given rng_state, its step word to step + 1.  ctl comes from new_accum_ctl(k, device)."""
    _chk(acc, "acc", torch.float32)
    _chk(g, "g", torch.float32)
    _chk(ctl, "ctl", torch.int32)
    n = acc.numel() if n is None else int(n)
    if n < 1 or n > acc.numel() or n > g.numel():
        raise ValueError(f"grad_accumulate: n = {n} does not fit acc ({acc.numel()}) and g ({g.numel()})")
    if ctl.numel() < 4:
        raise ValueError("grad_accumulate: ctl needs 4 words {j, k, arrival, 0} (new_accum_ctl)")
    if (loss is None) != (loss_out is None):
        raise ValueError("grad_accumulate: loss and loss_out go together")
    if loss is not None:
        _chk(loss, "loss", torch.float32)
        _chk(loss_out, "loss_out", torch.float32)
        if loss.numel() < 1 or loss_out.numel() < 2:
            raise ValueError("grad_accumulate: loss needs 1 float, loss_out 2 {sum, mean}")
    if rng_state is not None:
        _chk(rng_state, "rng_state", torch.int32)
        if rng_state.numel() < 4:
            raise ValueError("grad_accumulate: rng_state needs 4 words")
    check(lib.dg_grad_accumulate(_p(acc), _p(g), n, _p(ctl), _p(loss), _p(loss_out), _p(rng_state), _stream()), "dg_grad_accumulate")


def block_chain_supported(M: int, C: int, dtype: torch.dtype) -> bool:
    """can dg_block_chain_fwd run this shape?  (bf16 operands, C = 384, M % 64 == 0)"""
    return dtype == torch.bfloat16 and bool(lib.dg_block_chain_supported(int(M), int(C)))


def l2_warm(t: Tensor) -> None:
    """touch every 128-byte line of the contiguous tensor t from every XCD (its storage must start on a 128-byte boundary)"""
    _chk(t, "t")
    check(lib.dg_l2_warm(_p(t), t.numel() * t.element_size(), _stream()), "dg_l2_warm")


def pack_chain_weights(W: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """W [N, K] bf16 (N % 384 == 0, K % 32 == 0) -> the packed operand dg_block_chain_fwd streams (same shape / byte count)"""
    _chk(W, "W", torch.bfloat16, contiguous=False)
    N, K = W.shape
    if out is None:
        out = torch.empty((N, K), dtype=torch.bfloat16, device=W.device)
    _chk(out, "out", torch.bfloat16)
    check(lib.dg_pack_chain_weights(_p(W), _ld(W), _p(out), N, K, _stream()), "dg_pack_chain_weights")
    return out


def make_pack_table(pairs, device) -> tuple:
    """descriptor table for pack_chain_weights_batched: pairs = [(W [N, K] bf16, packed [N, K] bf16)]"""
    rows, first = [], 0
    for W, Pk in pairs:
        N, K = W.shape
        if N % 384 or K % 32:
            raise RuntimeError("pack_chain_weights: N % 384 == 0 and K % 32 == 0 required")
        rows.append([W.data_ptr(), Pk.data_ptr(), N, K, first, _ld(W)])
        first += (N // 384) * (K // 32)
    return torch.tensor(rows, dtype=torch.int64, device=device), len(rows), first


def pack_chain_weights_batched(table: Tensor, n_desc: int, total_stages: int) -> None:
    _chk(table, "table", torch.int64)
    check(lib.dg_pack_chain_weights_batched(_p(table), n_desc, total_stages, _stream()), "dg_pack_chain_weights_batched")


def block_chain_fwd(mode: int, M: int, Cd: int, *, o: Optional[Tensor] = None, x: Optional[Tensor] = None, wproj=None, bproj=None, ln2w=None, ln2b=None,
                    w1=None, b1=None, w2=None, b2=None, ln1w=None, ln1b=None, wqkv=None, f: Optional[Tensor] = None, x1: Optional[Tensor] = None,
                    dropout_p: float = 0.0, rng_state: Optional[Tensor] = None, site_proj: int = 0, site_ffn: int = 0, eps: float = 1e-5) -> dict:
    """row-local pieces of a residual block with the LayerNorm inside the producing GEMM's epilogue (dg_block_chain_fwd).
    mode 0: proj .. the next block's QKV in one launch; 1: last block (x2 comes back as bf16); 2: head (LayerNorm 1 + QKV of the
    first block on x); 3: proj + residual + LayerNorm 2 (o, x -> x1, h2, mean2, rstd2); 4: FFN2 + residual + the next block's
    LayerNorm 1 (f, x1 -> x2, h1, mean1, rstd1).  Weights are the PACKED bf16 operands (pack_chain_weights of the [out, in]
    matrices).  Returns the tensors the separate launches would have produced, by name."""
    from ._lib import BlockChainArgs
    dev = next(t for t in (x, o, f) if t is not None).device
    a = BlockChainArgs()
    a.mode, a.M, a.C, a.eps = mode, M, Cd, eps
    out = {}
    has_proj, has_ffn1, has_ffn2 = mode in (0, 1, 3), mode in (0, 1), mode in (0, 1, 4)
    has_qkv, ln1 = mode in (0, 2), mode in (0, 2, 4)

    def new(name, shape, dtype):
        t = out[name] = torch.empty(shape, dtype=dtype, device=dev)
        return t.data_ptr()

    def inp(t, name, dtype, n=None):
        _chk(t, name, dtype)
        if n is not None and t.numel() != n:
            raise RuntimeError(f"block_chain_fwd: {name} must hold {n} values, got {t.numel()}")
        return t.data_ptr()
    bf, f32 = torch.bfloat16, torch.float32
    if mode != 4:
        a.x = inp(x, "x", f32, M * Cd)
    if has_proj:
        a.o = inp(o, "o", bf, M * Cd)
        a.wproj, a.bproj = inp(wproj, "wproj", bf, Cd * Cd), inp(bproj, "bproj", f32, Cd)
        a.ln2w, a.ln2b = inp(ln2w, "ln2w", f32, Cd), inp(ln2b, "ln2b", f32, Cd)
        a.x1 = new("x1", (M, Cd), f32)
        a.mean2, a.rstd2 = new("mean2", (M,), f32), new("rstd2", (M,), f32)
        a.h2 = new("h2", (M, Cd), bf)
    if has_ffn1:
        a.w1, a.b1 = inp(w1, "w1", bf, 4 * Cd * Cd), inp(b1, "b1", f32, 4 * Cd)
        a.f = new("f", (M, 4 * Cd), bf)
        bits = out["bits"] = new_sign_bits(M, 4 * Cd, dev)
        a.sign_bits, a.sign_bits_bytes = bits.data_ptr(), bits.numel()
    if has_ffn2:
        if mode == 4:
            a.f, a.x1 = inp(f, "f", bf, M * 4 * Cd), inp(x1, "x1", f32, M * Cd)
        a.w2, a.b2 = inp(w2, "w2", bf, 4 * Cd * Cd), inp(b2, "b2", f32, Cd)
        if mode == 1:
            a.x2_bf16 = new("x2", (M, Cd), bf)
        else:
            a.x2 = new("x2", (M, Cd), f32)
    if ln1:
        a.ln1w, a.ln1b = inp(ln1w, "ln1w", f32, Cd), inp(ln1b, "ln1b", f32, Cd)
        a.mean1, a.rstd1 = new("mean1", (M,), f32), new("rstd1", (M,), f32)
        a.h1 = new("h1", (M, Cd), bf)
    if has_qkv:
        a.wqkv = inp(wqkv, "wqkv", bf, 3 * Cd * Cd)
        a.qkv = new("qkv", (M, 3 * Cd), bf)
    a.dropout_p = float(dropout_p)
    a.rng_state = _p(rng_state) if dropout_p > 0.0 else None
    a.site_proj, a.site_ffn = site_proj, site_ffn
    check(lib.dg_block_chain_fwd(C.byref(a), _stream()), "dg_block_chain_fwd")
    return out


def block_chain_bwd_supported(M: int, C: int, dtype: torch.dtype) -> bool:
    """can dg_block_chain_bwd run this shape?  (bf16 operands and gradient stream, C = 384, M % 64 == 0, M / 64 <= #CUs)"""
    return dtype == torch.bfloat16 and bool(lib.dg_block_chain_bwd_supported(int(M), int(C)))


def block_chain_bwd(mode: int, M: int, Cd: int, *, part_stride: int, dqkv=None, wqkvT=None, x=None, mean1=None, rstd1=None, ln1w=None, dresid1=None,
                    dln1w_part=None, dln1b_part=None, gbias1_part=None, g_in=None, w2T=None, bits=None, db1_part=None, w1T=None, x1=None,
                    mean2=None, rstd2=None, ln2w=None, dresid2=None, dln2w_part=None, dln2b_part=None, gbias2_part=None, wprojT=None,
                    dropout_p: float = 0.0, rng_state: Optional[Tensor] = None, site_ffn_below: int = 0, site_proj: int = 0) -> dict:
    """the backward pass's row-local chain between two attention-backward calls in one launch (dg_block_chain_bwd).
    mode 0: dX-QKV + LayerNorm-1 backward of block l, then dX-FFN2 / dX-FFN1 / LayerNorm-2 backward / dX-proj of block l - 1;
    1: the second half only (g_in = the operand of dX-FFN2); 2: the first half only.  Weights are the PACKED W^T operands
    (pack_chain_weights of the [in, out] shadows).  The *_part arguments are views of row 0 of a partial buffer with
    `part_stride` floats per row and at least 2 * M / 64 rows.  Returns the tensors the separate launches would have produced."""
    from ._lib import BlockChainBwdArgs
    a = BlockChainBwdArgs()
    a.mode, a.M, a.C = mode, M, Cd
    bf, f32 = torch.bfloat16, torch.float32
    has_q, has_2 = mode in (0, 2), mode in (0, 1)
    dev = (dqkv if has_q else g_in).device
    out = {}

    def new(name, shape, dtype=bf):
        t = out[name] = torch.empty(shape, dtype=dtype, device=dev)
        return t.data_ptr()

    def inp(t, name, dtype, n=None):
        _chk(t, name, dtype)
        if n is not None and t.numel() != n:
            raise RuntimeError(f"block_chain_bwd: {name} must hold {n} values, got {t.numel()}")
        return t.data_ptr()

    def part(t, name, n):
        _chk(t, name, f32, contiguous=False)
        if t.numel() != n:
            raise RuntimeError(f"block_chain_bwd: {name} must be a row of {n} partial sums, got {t.numel()}")
        return t.data_ptr()
    if has_q:
        a.dqkv, a.wqkvT = inp(dqkv, "dqkv", bf, M * 3 * Cd), inp(wqkvT, "wqkvT", bf, 3 * Cd * Cd)
        a.x, a.mean1, a.rstd1, a.ln1w = inp(x, "x", f32, M * Cd), inp(mean1, "mean1", f32, M), inp(rstd1, "rstd1", f32, M), inp(ln1w, "ln1w", f32, Cd)
        a.dresid1 = inp(dresid1, "dresid1", bf, M * Cd)
        a.dx1, a.g1 = new("dx1", (M, Cd)), new("g1", (M, Cd))
        a.dln1w_part, a.dln1b_part = part(dln1w_part, "dln1w_part", Cd), part(dln1b_part, "dln1b_part", Cd)
        a.gbias1_part = part(gbias1_part, "gbias1_part", Cd) if gbias1_part is not None else None
    if has_2:
        if mode == 1:
            a.g_in = inp(g_in, "g_in", bf, M * Cd)
        a.w2T, a.w1T, a.wprojT = inp(w2T, "w2T", bf, 4 * Cd * Cd), inp(w1T, "w1T", bf, 4 * Cd * Cd), inp(wprojT, "wprojT", bf, Cd * Cd)
        _chk(bits, "bits", torch.uint8)
        a.sign_bits, a.sign_bits_bytes = bits.data_ptr(), bits.numel()
        a.df = new("df", (M, 4 * Cd))
        a.db1_part = part(db1_part, "db1_part", 4 * Cd)
        a.x1, a.mean2, a.rstd2, a.ln2w = inp(x1, "x1", f32, M * Cd), inp(mean2, "mean2", f32, M), inp(rstd2, "rstd2", f32, M), inp(ln2w, "ln2w", f32, Cd)
        a.dresid2 = out["dx1"].data_ptr() if mode == 0 else inp(dresid2, "dresid2", bf, M * Cd)
        a.dx2, a.g2, a.dout = new("dx2", (M, Cd)), new("g2", (M, Cd)), new("dout", (M, Cd))
        a.dln2w_part, a.dln2b_part = part(dln2w_part, "dln2w_part", Cd), part(dln2b_part, "dln2b_part", Cd)
        a.gbias2_part = part(gbias2_part, "gbias2_part", Cd)
    a.part_stride = int(part_stride)
    a.dropout_p = float(dropout_p)
    a.rng_state = _p(rng_state) if dropout_p > 0.0 else None
    a.site_ffn_below, a.site_proj = site_ffn_below, site_proj
    check(lib.dg_block_chain_bwd(C.byref(a), _stream()), "dg_block_chain_bwd")
    return out
